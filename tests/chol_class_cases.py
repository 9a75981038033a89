"""Small SPD systems whose fronts are known in advance, for the small-front Cholesky kernels (test_chol_classes_cpu.py pins the
designs on the host, test_chol_classes_gpu.py runs them).  Not a conftest: plain helpers.

A system is a list of dense blocks (k, below): k columns, dense among themselves, each with the same explicit rows `below` (global
column numbers of later blocks).  Analysed in natural order with every amalgamation off (OPTS) the blocks come out as the fronts,
up to the renumbering of the postorder, because

  * column j joins column j - 1 when j is its parent and the column counts nest (symbolic.cpp, step 4) -- also when j has other
    children; a block whose rows are ALL the rows of the column it touches first is therefore absorbed unless another, larger
    child of that column stands between them in the postorder (children by increasing subtree size; of equal size the larger
    index first);
  * a block stays whole only if, at each of its columns, the part of the block before it is the largest child.

leaf(m, k): a leaf front of exactly m rows and k pivots under a dense separator of u + 2 columns (u = m - k > 0).  The leaf touches
the separator's second column and its last u - 1, a one-column companion its first column.  The leaf's rows are then not those of
the column it hangs under, and it is not absorbed.  The separator's second column has two children, its first column (with the
companion: 2 columns) and the leaf (k columns): with k < 2 the first column is the larger child and the separator stays whole,
fronts (m, k, 0), (2, 1, 0), (u + 2, u + 2, 2); from k = 2 on the leaf stands between them and the first column is a front of its own,
(m, k, 0), (2, 1, 0), (u + 2, 1, 1), (u + 1, u + 1, 2).  That front of one pivot sits on the leaf's level; it is of a k <= 16 / k <= 32
class and changes no template size of a launch there.
"""
import numpy as np

OPTS = {"ordering": 1, "relax_small": 0, "relax_z1": 0.0, "relax_z2": 0.0, "relax_z3": 0.0, "leaf_cols": 0}

CLS_BIG, CLS_LDS128, CLS_LDS96, CLS_WAVE0 = 0, 1, 2, 3
CLASS_NAMES = ("big", "lds128", "lds96", "wave64_k32", "wave64_k16", "wave48_k32", "wave48_k16", "wave32_k32", "wave32_k16")


def front_class(m, k):
    """symbolic.hpp front_class, restated"""
    if m > 128 or k > 64:
        return CLS_BIG
    if m > 64 or k > 32:
        return CLS_LDS128 if m > 96 else CLS_LDS96
    mc = 2 if m <= 32 else (1 if m <= 48 else 0)
    return CLS_WAVE0 + 2 * mc + (1 if k <= 16 else 0)


def wave_image(m):
    return 32 if m <= 32 else (48 if m <= 48 else 64)


class Design:
    """blocks with rows relative to the design's first column, the fronts they must give, what the design is for"""

    def __init__(self, blocks, fronts, tags=()):
        self.blocks, self.fronts, self.tags = blocks, fronts, list(tags)
        self.n = sum(k for k, _ in blocks)


def root(m):
    return Design([(m, [])], [(m, m, 0)], [("leaf", m, m), ("u", 0)])


def _top(u, cols_below):
    """fronts of the companion and the separator above a front with u update rows and cols_below columns in its subtree"""
    return [(2, 1, 0), (u + 2, u + 2, 2)] if cols_below < 2 else [(2, 1, 0), (u + 2, 1, 1), (u + 1, u + 1, 2)]


def leaf(m, k):
    u = m - k
    assert u > 0
    sep = k + 1
    below = [sep + 1] + list(range(sep + 3, sep + u + 2))
    return Design([(k, below), (1, [sep]), (u + 2, [])], [(m, k, 0)] + _top(u, k), [("leaf", m, k), ("u", u)])


def family(mp, kp, children, tags=()):
    """A front (mp, kp) with its own Schur complement, under a companion and a dense root as in leaf(), and below it one leaf per
    entry (kc, rows) of children: kc pivots whose update rows are the given rows of the parent front (0 .. mp - 1, in front order).
    The rows of the first (largest) child start at 0 so that the parent's first column is not split off."""
    up = mp - kp
    assert up > 0
    nc = sum(kc for kc, _ in children)
    p0 = nc
    sep = p0 + kp + 1
    prow = list(range(p0, p0 + kp)) + [sep + 1] + list(range(sep + 3, sep + up + 2))      # global column of every parent row
    blocks, fronts = [], []
    for kc, rows in children:
        assert rows == sorted(set(rows)) and rows[0] < kp and rows[-1] < mp
        blocks.append((kc, [prow[r] for r in rows]))
        fronts.append((kc + len(rows), kc, 0))
    blocks += [(kp, prow[kp:]), (1, [sep]), (up + 2, [])]
    fronts += [(mp, kp, len(children))] + _top(up, nc + kp)
    t = [("parent", front_class(mp, kp), len(children)), ("u", up)]
    for kc, rows in children:
        t += [("child_u", front_class(mp, kp), len(rows)), ("u", len(rows))]
        if rows != list(range(mp - len(rows), mp)):
            t.append(("scattered", front_class(mp, kp)))
        if rows[0] == 0:
            t.append(("first_row", front_class(mp, kp)))
        if rows[-1] == mp - 1:
            t.append(("last_row", front_class(mp, kp)))
    return Design(blocks, fronts, t + list(tags))


def star(kroot, leaves):
    """A root of kroot columns with one leaf per entry of leaves (columns; each touches the root's first and last column): a tree of
    wave fronts that is one leaf subtree of the sweeps, or too large for one."""
    nc = sum(leaves)
    blocks = [(kc, [nc, nc + kroot - 1]) for kc in leaves] + [(kroot, [])]
    fronts = [(kc + 2, kc, 0) for kc in leaves] + [(kroot, kroot, len(leaves))]
    return Design(blocks, fronts, [("u", 2)])


class Case:
    def __init__(self, name, designs, env=None, tags=(), subtrees=None):
        self.name, self.designs, self.env = name, designs, dict(env or {})
        self.tags = [t for d in designs for t in d.tags] + list(tags)
        self.fronts = sorted(f for d in designs for f in d.fronts)
        self.n = sum(d.n for d in designs)
        self.subtrees = subtrees          # (subtrees, fronts inside) the analysis must report under env, where the case pins it
        self.seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))

    @property
    def all_small(self):
        return all(front_class(m, k) != CLS_BIG for m, k, _ in self.fronts)

    def system(self, seed=None):
        """n, colptr, rowind, values of the lower triangle (int64 / float64): off-diagonals in [-1, -0.25] u [0.25, 1], every
        diagonal the sum of the absolute values of its row plus something in [0.5, 1.5]"""
        rng = np.random.default_rng(self.seed if seed is None else seed)
        cols, base = [], 0
        for d in self.designs:
            s = base
            for k, below in d.blocks:
                for j in range(s, s + k):
                    cols.append(list(range(j, s + k)) + [base + r for r in below])
                s += k
            base += d.n
        n = base
        cp = np.zeros(n + 1, dtype=np.int64)
        for j, c in enumerate(cols):
            assert c == sorted(c) and c[0] == j and c[-1] < n, (self.name, j)
            cp[j + 1] = cp[j] + len(c)
        ri = np.array([r for c in cols for r in c], dtype=np.int64)
        vx = rng.uniform(0.25, 1.0, ri.size) * rng.choice([-1.0, 1.0], ri.size)
        rowsum = np.zeros(n)
        col = np.repeat(np.arange(n), np.diff(cp))
        off = ri != col
        np.add.at(rowsum, ri[off], np.abs(vx[off]))
        np.add.at(rowsum, col[off], np.abs(vx[off]))
        vx[cp[:-1]] = rowsum + rng.uniform(0.5, 1.5, n)
        return n, cp, ri, vx

    def trees(self):
        """(first column, columns) of every design in the caller's numbering: the system is block diagonal over them"""
        out, base = [], 0
        for d in self.designs:
            out.append((base, d.n))
            base += d.n
        return out


def dense_lower(n, cp, ri, vx, dtype=np.float64):
    """the symmetric matrix of a lower-triangle CCS"""
    A = np.zeros((n, n), dtype=dtype)
    col = np.repeat(np.arange(n), np.diff(cp))
    A[ri, col] = vx
    A[col, ri] = vx
    return A


WAVE_M = (1, 2, 16, 17, 32, 33, 48, 49, 64)
WAVE_K = (1, 2, 3, 5, 16, 17, 32)
LDS96_LEAVES = ((64, 33), (65, 1), (65, 64), (96, 32), (96, 33), (96, 64))
LDS128_LEAVES = ((97, 1), (97, 64), (128, 1), (128, 32), (128, 33), (128, 63), (128, 64))


def _one(m, k):
    return root(m) if m == k else leaf(m, k)


def _spread(mp, count, first, last):
    """count rows of a front of mp rows, spread out, not a tail: with row 0 if first, with the last row if last"""
    assert count <= mp
    if count == mp:
        return list(range(mp))
    lo, hi = (0 if first else 1), (mp - 1 if last else mp - 2)
    if count == 1:
        return [lo if first or not last else hi]
    rows = sorted(set(int(round(lo + i * (hi - lo) / (count - 1))) for i in range(count)))
    assert len(rows) == count
    return rows


def _cases():
    C = []
    # ---- leaf fronts, one system per kernel class so that each launch keeps the instantiation of its class
    by_cls = {}
    for m in WAVE_M:
        for k in WAVE_K:
            if k <= m:
                by_cls.setdefault(front_class(m, k), []).append((m, k))
    for cls, mk in sorted(by_cls.items()):
        # the root of a leaf with more than 62 update rows is a big front: those leaves get a system of their own
        small = [x for x in mk if x[0] - x[1] <= 62]
        wide = [x for x in mk if x[0] - x[1] > 62]
        C.append(Case("leaves_" + CLASS_NAMES[cls], [_one(m, k) for m, k in small]))
        if wide:
            C.append(Case("leaves_" + CLASS_NAMES[cls] + "_bigroot", [_one(m, k) for m, k in wide]))
    C.append(Case("leaves_lds96_k32", [leaf(65, 1), leaf(96, 32)]))
    C.append(Case("leaves_lds96_k64", [leaf(64, 33), leaf(65, 64), leaf(96, 33), leaf(96, 64)]))
    C.append(Case("leaves_lds128_k32", [leaf(97, 1), leaf(128, 32)]))
    C.append(Case("leaves_lds128_k64", [leaf(97, 64), leaf(128, 33), leaf(128, 63), leaf(128, 64)]))
    C.append(Case("leaves_lds128_bigroot", [leaf(128, 1)]))
    C.append(Case("leaves_big", [leaf(129, 1), root(65)]))
    # ---- roots and leaves without a Schur complement inside a forest: u = 0 next to trees with parents
    C.append(Case("forest_u0", [root(1), root(5), root(17), leaf(17, 16), root(33), root(64), leaf(20, 4)]))
    # ---- Schur complements the leaf grid does not give: u = 1 .. 127
    C.append(Case("schur_small", [leaf(34, 33), leaf(20, 5), leaf(36, 20), leaf(50, 33), leaf(40, 9)]))      # u = 1, 15, 16, 17, 31
    C.append(Case("schur_wide", [leaf(96, 33), leaf(100, 36), leaf(128, 1)]))                                # u = 63, 64, 127
    # ---- fronts with children
    C.append(Case("kids_wave1", [family(32, 8, [(3, _spread(32, 9, True, True))])]))
    C.append(Case("kids_wave48_2", [family(48, 17, [(5, _spread(48, 17, True, True)), (2, _spread(48, 16, False, False))])]))
    C.append(Case("kids_lds128_1", [family(128, 33, [(3, _spread(128, 40, True, True))])]))
    C.append(Case("kids_lds96_2", [family(80, 33, [(6, _spread(80, 33, True, False)), (2, _spread(80, 32, False, True))])]))
    C.append(Case("kids_wave5", [family(64, 20, [(9, _spread(64, 33, True, False)), (2, _spread(64, 64, True, True)), (4, _spread(64, 17, False, True)),
                                                 (3, _spread(64, 16, True, False)), (1, [5])])]))
    C.append(Case("kids_lds96_5", [family(96, 40, [(9, _spread(96, 65, True, True)), (5, _spread(96, 64, False, False)), (4, _spread(96, 33, True, False)),
                                                   (3, _spread(96, 32, False, True)), (1, [7])])]))
    C.append(Case("kids_lds128_6", [family(128, 40, [(9, _spread(128, 65, True, True)), (2, _spread(128, 128, True, True)),
                                                     (5, _spread(128, 64, False, False)), (4, _spread(128, 33, True, False)),
                                                     (3, _spread(128, 32, False, True)), (1, [11])])]))
    # ---- mixed levels: lists of both template sizes meet in one launch
    C.append(Case("mixed_lds96", [leaf(70, 20), leaf(70, 40)], tags=[("mixed", "lds96")]))
    C.append(Case("mixed_lds128", [leaf(110, 20), leaf(110, 50)], tags=[("mixed", "lds128")]))
    C.append(Case("mixed_wave48", [leaf(40, 5), leaf(40, 20)], tags=[("mixed", "wave48")]))
    C.append(Case("mixed_wave32", [leaf(30, 5), leaf(30, 20)], tags=[("mixed", "wave32")]))
    C.append(Case("mixed_wave64", [leaf(60, 5), leaf(60, 20)], tags=[("mixed", "wave64")]))
    # ---- three copies of one leaf design per small class: every launch numbers at least three fronts
    reps = [(20, 5), (30, 20), (40, 5), (40, 20), (60, 5), (60, 20), (70, 40), (110, 50)]
    C.append(Case("forest3", [leaf(m, k) for m, k in reps for _ in range(3)], tags=[("forest3",)]))
    # ---- limits of the leaf subtrees of the sweeps (device.hpp): fronts per subtree (KVX_SUB_MAXF, 4 by default below order
    # 150 000, 12 above) and pivot columns per subtree (KVX_SUB_MAXCOLS = 256)
    C.append(Case("sub_f4", [star(4, [1, 2, 3])], subtrees=(1, 4), tags=[("sub_fronts", 4)]))
    C.append(Case("sub_f5", [star(4, [1, 2, 3, 4])], subtrees=(4, 4), tags=[("sub_fronts", 5)]))
    C.append(Case("sub_f12", [star(4, list(range(1, 12)))], env={"KVX_SUB_MAXF": "12"}, subtrees=(1, 12), tags=[("sub_fronts", 12)]))
    C.append(Case("sub_f13", [star(4, list(range(1, 13)))], env={"KVX_SUB_MAXF": "12"}, subtrees=(12, 12), tags=[("sub_fronts", 13)]))
    C.append(Case("sub_c256", [star(32, [26, 27, 28, 29, 30, 31, 32, 21])], env={"KVX_SUB_MAXF": "12"}, subtrees=(1, 9), tags=[("sub_cols", 256)]))
    C.append(Case("sub_c257", [star(32, [26, 27, 28, 29, 30, 31, 32, 22])], env={"KVX_SUB_MAXF": "12"}, subtrees=(8, 8), tags=[("sub_cols", 257)]))
    return C


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def realised(F):
    """per front of an analysed factor, in its numbering: (m, k, children), level, parent, first column"""
    sup, nrows, parent, level = F.supernodes()
    ns = len(nrows)
    nch = np.bincount(parent[parent >= 0], minlength=ns) if ns else np.zeros(0, dtype=np.int64)
    fronts = [(int(nrows[s]), int(sup[s + 1] - sup[s]), int(nch[s])) for s in range(ns)]
    return fronts, [int(x) for x in level], [int(x) for x in parent], [int(x) for x in sup]


SUB_MAXCOLS, SUB_STACK = 256, 512


def pick_subtrees(fronts, parent, sup, maxf):
    """chol_setup.cpp pick_subtrees, restated: the leaf subtrees [lo, hi] of the sweeps (maximal subtrees of wave fronts, at most maxf
    fronts and SUB_MAXCOLS pivot columns, update vectors within the LDS stack)"""
    ns = len(fronts)
    kids = [[] for _ in range(ns)]
    for s, p in enumerate(parent):
        if p >= 0:
            kids[p].append(s)
    cnt, lo_of, ok = [1] * ns, list(range(ns)), [False] * ns
    for s in range(ns):
        good = front_class(fronts[s][0], fronts[s][1]) >= CLS_WAVE0
        for c in kids[s]:
            good = good and ok[c]
            cnt[s] += cnt[c]
            lo_of[s] = min(lo_of[s], lo_of[c])
        lo = s - cnt[s] + 1
        ok[s] = good and cnt[s] <= maxf and lo_of[s] == lo and sup[s + 1] - sup[lo] <= SUB_MAXCOLS
    subs = []
    for s in range(ns - 1, -1, -1):
        if not ok[s] or (parent[s] >= 0 and ok[parent[s]]):
            continue
        lo, sp, top, fits = s - cnt[s] + 1, 0, 0, True
        for q in range(lo, s + 1):
            sp -= sum(fronts[c][0] - fronts[c][1] for c in kids[q])
            fits = fits and sp >= 0
            if q != s:
                sp += fronts[q][0] - fronts[q][1]
            top = max(top, sp)
        if fits and top <= SUB_STACK:
            subs.append((lo, s))
    return subs


def default_maxf(n, env):
    return max(1, min(int(env["KVX_SUB_MAXF"]), 48)) if "KVX_SUB_MAXF" in env else (4 if n <= 150000 else 12)


# ---- the factor's figure of merit, in longdouble, tree by tree (the systems are block diagonal over their designs) -------------
LD = np.longdouble
U = LD(2.0) ** -53


def dense_factor(n, Lp, Li, Lx):
    L = np.zeros((n, n))
    L[Li, np.repeat(np.arange(n), np.diff(Lp))] = Lx
    return L


def tree_ranges(case, ip):
    out = []
    for first, cols in case.trees():
        a = int(ip[first:first + cols].min())
        out.append((a, a + cols))
    return out


def rho_of(C, L, ranges):
    """max over the lower triangle of |P A P' - L L'| / (2^-53 |L| |L|')"""
    worst = 0.0
    for a, b in ranges:
        Lb = L[a:b, a:b].astype(LD)
        R = np.abs(C[a:b, a:b].astype(LD) - Lb @ Lb.T)
        S = U * (np.abs(Lb) @ np.abs(Lb).T)
        low = np.tril(np.ones(R.shape, dtype=bool))
        assert np.all(R[low & (S == 0)] == 0)
        ok = low & (S > 0)
        worst = max(worst, float((R[ok] / S[ok]).max()))
    return worst
