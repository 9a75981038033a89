"""Cases, references and bounds for the orthant KKT-step kernels of csrc/kkt.hip at their lane, workgroup and grid edges
(tests/test_kkt_edges_cpu.py checks the cases and the bound on the host, tests/test_kkt_edges_gpu.py asks them of the device).
Nothing here touches the device library.

The bound.  Every reference below restates the formula in the kernel's comment in numpy.longdouble and returns, per output entry,
    ref   the value,
    T     the value of the same formula with every term replaced by its absolute value (the sum of the absolute terms),
    K     the number of terms of the sum behind the entry (for the fixed-tree reductions: the depth of the tree).
An entry passes when |got - ref| <= (K + R) 2^-52 T, with R the number of roundings outside the sum, counted from the kernel's
source and stated at each reference.  2^-52 is twice the unit roundoff: the factor two absorbs the second-order terms of the
standard forward bound (1 + u)^k - 1 <= k u / (1 - k u).  A sum of K terms in ANY order rounds at most K - 1 times on the way of
any one term (an addition of an exact zero does not round), so K terms cover the 4-, 8- and 16-lane forms, the one-, two- and
four-lane product lists and the atomics alike.  Operands that are divided by or whose root is taken are drawn positive, so that T
is the magnitude of the quotient's or root's argument and the count of roundings carries through.  The bound is derived, never
measured: test_kkt_edges_cpu.py asserts that plain float64 numpy lies inside it before it is asked of the device.

Data have no exact zeros and magnitudes spread over [1e-3, 1e3] (log-uniform): a dropped or doubled term moves an entry by
orders of magnitude more than the bound.

Every function of the form f(D, ...) evaluates in the dtype D: with D = LD it is the reference, with D = np.float64 the
correctly rounded evaluation the bound must admit."""
import collections

import numpy as np

LD = np.longdouble
F8 = np.float64
U = 2.0 ** -52
PAD = 64                                       # sentinel doubles behind every device buffer
SENTINEL = -1.2345678901234567e+300            # (finite: compared by its bits)
RED_BLOCKS = 256
CAP_GRID = 2048                                # grid_for
CAP_GROUPS = 16384                             # groups16
CAP_POST_X = 4096                              # launch_kkt_post, x part
CAP_SPMM = 4096                                # launch_spmm_t

Out = collections.namedtuple("Out", "ref T K R")       # K: array or scalar; R: scalar


def spread(rng, n, signed=True):
    """n values with magnitudes log-uniform in [1e-3, 1e3], no zeros"""
    v = 10.0 ** rng.uniform(-3.0, 3.0, int(n))
    if signed:
        v *= np.where(rng.random(int(n)) < 0.5, -1.0, 1.0)
    return v


def ratio(got, out):
    """largest |got - ref| / bound over the entries; an entry whose bound is zero must be met exactly (ratio 0 or inf)"""
    got = np.asarray(got, dtype=F8).reshape(-1)
    ref = np.asarray(out.ref, dtype=LD).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    assert np.all(np.isfinite(got)), "non-finite entries at %s" % np.flatnonzero(~np.isfinite(got))[:5]
    bound = (np.asarray(out.K, dtype=LD).reshape(-1) + LD(out.R)) * LD(U) * np.asarray(out.T, dtype=LD).reshape(-1)
    bound = np.broadcast_to(bound, ref.shape)
    err = np.abs(got.astype(LD) - ref)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=F8).reshape(-1)
    b = np.ascontiguousarray(b, dtype=F8).reshape(-1)
    return a.shape == b.shape and bool(np.all(a.view(np.int64) == b.view(np.int64)))


# ---- 1. elementwise kernels -------------------------------------------------------------------------------------------------
ELEM_SIZES = [1, 255, 256, 257, 524288, 524289, 1048577]


def elem_data(n, seed=11):
    rng = np.random.default_rng(seed + n)
    pos = lambda: spread(rng, n, signed=False)
    sgn = lambda: spread(rng, n)
    return dict(s=pos(), z=pos(), d=pos(), lm=pos(), lsq=pos(), ws3=sgn(), rz=sgn(), z1=sgn(), ds=sgn(), dz=sgn(), x=sgn(), y=sgn(),
                zz=sgn(), dsp=pos(), dzp=pos(), shift=0.37109375, scale=-0.8125, dtau=0.6328125, step=0.59375, a=-1.75, b=0.4375,
                c=3.0625)


def e_compute_scaling(D, s, z):
    """d = sqrt(s / z): R = 2; di = 1 / d: R = 3; lmbda = sqrt(s z): R = 2.  s, z > 0: T = |ref|."""
    s, z = s.astype(D), z.astype(D)
    d = np.sqrt(s / z)
    di = 1 / d
    lm = np.sqrt(s * z)
    return dict(d=Out(d, abs(d), 0, 2), di=Out(di, abs(di), 0, 3), lm=Out(lm, abs(lm), 0, 2))


def e_update_scaling(D, s, z, d):
    """s := sqrt(s), z := sqrt(z): R = 1; d := (d s) / z: R = 4; di := 1 / d: R = 5; lmbda := s z: R = 3.  All positive."""
    ss, zz = np.sqrt(s.astype(D)), np.sqrt(z.astype(D))
    dd = (d.astype(D) * ss) / zz
    di = 1 / dd
    lm = ss * zz
    return dict(s=Out(ss, ss, 0, 1), z=Out(zz, zz, 0, 1), d=Out(dd, dd, 0, 4), di=Out(di, di, 0, 5), lm=Out(lm, lm, 0, 3))


def e_newton_rhs(D, lsq, ws3, shift, scale, rz, lm, d):
    """ds := -(lmbdasq (+ ws3 - shift)) ./ lmbda ; dz := -(scale rz + d .* ds).  lmbdasq NULL: lmbda o lmbda, one rounding more.
    R(ds) = [1 if lsq is None] + [2 if ws3 is given] + 1 (the division); R(dz) = R(ds) + 3 (two products, one addition)."""
    lm, d, rz = lm.astype(D), d.astype(D), rz.astype(D)
    r = 1
    if lsq is None:
        v = lm * lm
        r += 1
    else:
        v = lsq.astype(D)
    tv = abs(v)
    if ws3 is not None:
        v = (v + ws3.astype(D)) - D(shift)
        tv = tv + abs(ws3.astype(D)) + abs(D(shift))
        r += 2
    v = -(v / lm)
    tv = tv / abs(lm)
    dz = -(D(scale) * rz + v * d)
    return dict(ds=Out(v, tv, 0, r), dz=Out(dz, abs(D(scale) * rz) + tv * abs(d), 0, r + 3))


def e_step_post(D, dtau, z1, lm, ds, dz, want_ws3=True):
    """zz = dz + dtau z1 (R 2); ss = ds - zz (R 3); ws3 := ss .* zz (R 6); ds := ss / lmbda (R 4); dz := zz / lmbda (R 3)."""
    z1, lm, ds, dz = z1.astype(D), lm.astype(D), ds.astype(D), dz.astype(D)
    zz = dz + D(dtau) * z1
    tz = abs(dz) + abs(D(dtau) * z1)
    ss = ds - zz
    ts = abs(ds) + tz
    out = dict(ds=Out(ss / lm, ts / abs(lm), 0, 4), dz=Out(zz / lm, tz / abs(lm), 0, 3))
    if want_ws3:
        out["ws3"] = Out(ss * zz, ts * tz, 0, 6)
    return out


def e_lp_update(D, step, ds, dz, d, lm):
    """ds := sqrt((step ds + 1) lmbda) (R 4), dz likewise; d := (d ds) / dz (R 10); di := 1 / d (R 11); lmbda := ds dz (R 9);
    s := lmbda d (R 20); z := lmbda di (R 21).  step, ds, dz > 0: no cancellation under the roots, T = |ref|."""
    ds, dz, d, lm = ds.astype(D), dz.astype(D), d.astype(D), lm.astype(D)
    ss = np.sqrt((D(step) * ds + 1) * lm)
    zz = np.sqrt((D(step) * dz + 1) * lm)
    dd = (d * ss) / zz
    di = 1 / dd
    ln = ss * zz
    s, z = ln * dd, ln * di
    return dict(ds=Out(ss, ss, 0, 4), dz=Out(zz, zz, 0, 4), d=Out(dd, dd, 0, 10), di=Out(di, di, 0, 11), lm=Out(ln, ln, 0, 9),
                s=Out(s, s, 0, 20), z=Out(z, z, 0, 21))


def e_mul(D, x, y):
    """x .* y: R = 1 (scale, scale2 inverse, sprod, ssqr with y = x)"""
    v = x.astype(D) * y.astype(D)
    return Out(v, abs(v), 0, 1)


def e_div(D, x, y):
    """x ./ y: R = 1 (scale2, sinv)"""
    v = x.astype(D) / y.astype(D)
    return Out(v, abs(v), 0, 1)


def e_axpy(D, alpha, x, y):
    """y + alpha x: R = 2"""
    ax = D(alpha) * x.astype(D)
    return Out(y.astype(D) + ax, abs(y.astype(D)) + abs(ax), 0, 2)


def e_lincomb(D, a, x, b, y):
    """a x + b y: R = 2 (a x, then fma(b, y, .)); b == 0: a x, R = 1, y not read"""
    ax = D(a) * x.astype(D)
    if b == 0:
        return Out(ax, abs(ax), 0, 1)
    by = D(b) * y.astype(D)
    return Out(ax + by, abs(ax) + abs(by), 0, 2)


def e_scal(D, alpha, x):
    v = D(alpha) * x.astype(D)
    return Out(v, abs(v), 0, 1)


def e_addc(D, c, x):
    return Out(x.astype(D) + D(c), abs(x.astype(D)) + abs(D(c)), 0, 1)


def e_xmy(D, a, x, y, b, z):
    """a (x .* y) + b z: R = 4; b == 0: R = 2, z not read"""
    t = D(a) * (x.astype(D) * y.astype(D))
    if b == 0:
        return Out(t, abs(t), 0, 2)
    bz = D(b) * z.astype(D)
    return Out(t + bz, abs(t) + abs(bz), 0, 4)


# ---- 2. reductions ------------------------------------------------------------------------------------------------------------
RED_SIZES = [1, 63, 64, 255, 256, 257, 65535, 65536, 65537, 524289]


def red_per(n):
    return -(-n // RED_BLOCKS)


def red_depth(n):
    """additions on the way of one term through k_reduce1 / k_reduce2: ceil(per / 256) serial steps of a thread, 6 butterfly
    steps, 3 across the waves; 4 serial steps and 6 butterfly steps in stage two"""
    return -(-red_per(n) // 256) + 6 + 3 + 4 + 6


def r_dot(D, x, y):
    """sum_i x_i y_i on the fixed tree: K = red_depth(n), R = 1 (the product, where it is not fused into the addition)"""
    t = x.astype(D) * y.astype(D)
    return Out(np.array([t.sum(dtype=D)]), np.array([abs(t).sum(dtype=D)]), red_depth(len(x)), 1)


def r_max_step(x):
    """max_i(-x_i): exact"""
    return float(np.max(-x))


def red_data(n, seed=23):
    rng = np.random.default_rng(seed + n)
    return spread(rng, n), spread(rng, n)


def max_step_plants(n):
    """indices at which the extreme element is planted, one case each: 0, n - 1, the last index of a workgroup's chunk, the first of
    the next chunk, b0 + 256 (the first element of a thread's second trip); those that n does not have are left out"""
    per = red_per(n)
    c = min(3, (n - 1) // per)                        # a chunk in the middle of the grid where there is one
    b0 = c * per
    pl = {"first": 0, "last": n - 1}
    if c > 0:
        pl["chunk_end"] = b0 - 1
        pl["chunk_start"] = b0
    if per > 256 and b0 + 256 < n:
        pl["second_trip"] = b0 + 256
    return pl


def multi_cases():
    """(name, [(kind, n)]) for kvx_nt_reduce_multi_dev: counts 1, 7 and 32, mixed kinds, different n per slot, one slot with n = 0"""
    sizes = [257, 5, 65537, 1, 64, 255, 256, 63, 65536, 65535, 524289]
    return [("count1", [(0, 257)]),
            ("count7", [(0, 257), (0, 0), (1, 65537), (0, 1), (1, 64), (0, 65537), (1, 255)]),
            ("count32", [(k % 2, sizes[k % len(sizes)]) for k in range(32)])]


# ---- 3. CCS products --------------------------------------------------------------------------------------------------------
def ccs_by_lengths(rng, m, lens):
    """CCS arrays of an m-row matrix (m prime or 1) whose column j holds lens[j] entries in distinct rows, ascending"""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.max(initial=0) <= m
    n = len(lens)
    cp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.repeat(np.arange(n, dtype=np.int64), lens)
    k = np.arange(cp[-1], dtype=np.int64) - cp[col]
    start = rng.integers(0, m, n)
    stride = rng.integers(1, m, n) if m > 1 else np.zeros(n, dtype=np.int64)
    ri = (start[col] + k * stride[col]) % m
    order = np.lexsort((ri, col))
    ri = np.ascontiguousarray(ri[order], dtype=np.int64)
    assert np.all((np.diff(ri) > 0) | (np.diff(col) > 0))
    return cp, ri, spread(rng, cp[-1])


def transpose_ccs(m, n, cp, ri, vx):
    """CCS arrays of the transpose (rows of the original, columns ascending within a row)"""
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    order = np.argsort(ri, kind="stable")
    tp = np.zeros(m + 1, dtype=np.int64)
    if len(ri):
        np.cumsum(np.bincount(ri, minlength=m), out=tp[1:])
    return tp, np.ascontiguousarray(col[order]), np.ascontiguousarray(vx[order])


def gather_sum(D, n, cp, terms):
    """per column j the sum of terms[cp[j]:cp[j + 1]] in D (empty: 0)"""
    out = np.zeros(n, dtype=D)
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    np.add.at(out, col, terms.astype(D))
    return out


SPMV_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 100]
SPMV_AB = [(1.0, 0.0), (-1.0, 1.0), (2.0, -0.5)]

Mat = collections.namedtuple("Mat", "name m n cp ri vx")


def lens_cycle(n, lens, empty_ends=True):
    out = np.array([lens[j % len(lens)] for j in range(n)], dtype=np.int64)
    if empty_ends and n >= 2:
        out[0] = out[-1] = 0
    return out


def spmv_t_mats(seed=31):
    """'T' cases: n in {1, 16, 17, 32769}; column lengths cycle through SPMV_LENS, the first and the last column empty (n = 1: one
    column of 33); 32769 columns of 16 lanes are one group more than grid_for's 2048 workgroups hold"""
    rng = np.random.default_rng(seed)
    mats = []
    for n in (1, 16, 17, 32769):
        lens = lens_cycle(n, SPMV_LENS[1:] + SPMV_LENS[:1]) if n > 1 else np.array([33])
        m = 127
        cp, ri, vx = ccs_by_lengths(rng, m, lens)
        mats.append(Mat("t%d" % n, m, n, cp, ri, vx))
    return mats


def spmv_n_mats(seed=37):
    """'N' cases: the 'T' matrices, a matrix with a row of 300 entries, and 524289 columns of one entry each (one more than
    grid_for's 2048 x 256 threads)"""
    rng = np.random.default_rng(seed)
    mats = list(spmv_t_mats())
    # rows of lengths (300, 0, 1, 17, ...) by building the transpose by its column lengths
    rl = lens_cycle(40, [300, 1, 17, 33, 2], empty_ends=False)
    rl[1] = 0
    tp, ti, tx = ccs_by_lengths(rng, 307, rl)                    # 40 x 307 transposed: the matrix is 40 rows, 307 columns
    cp, ri, vx = transpose_ccs(307, 40, tp, ti, tx)
    mats.append(Mat("row300", 40, 307, cp, ri, vx))
    n = 524289
    cp, ri, vx = ccs_by_lengths(rng, 1031, np.ones(n, dtype=np.int64))
    mats.append(Mat("n524289", 1031, n, cp, ri, vx))
    return mats


def spmm_mat(seed=41):
    """65537 columns (cap 4096 workgroups of 16 groups = 65536), lengths cycling through {0, 1, 2, 16, 17}"""
    rng = np.random.default_rng(seed)
    n = 65537
    cp, ri, vx = ccs_by_lengths(rng, 127, lens_cycle(n, [1, 2, 16, 17, 0]))
    return Mat("spmm65537", 127, n, cp, ri, vx)


def c_spmv_t(D, mat, alpha, x, beta, y):
    """y_j := beta y_j + alpha <A(:, j), x>: K = entries of the column, R = 4 (product of a term, alpha acc, beta y, the addition);
    beta == 0: y not read, R = 2"""
    t = mat.vx.astype(D) * x.astype(D)[mat.ri]
    acc = gather_sum(D, mat.n, mat.cp, t)
    ta = gather_sum(D, mat.n, mat.cp, abs(t))
    K = np.diff(mat.cp)
    if beta == 0:
        return Out(D(alpha) * acc, abs(D(alpha)) * ta, K, 2)
    by = D(beta) * y.astype(D)
    return Out(by + D(alpha) * acc, abs(by) + abs(D(alpha)) * ta, K, 4)


def c_spmv_n(D, mat, alpha, x, beta, y):
    """y_i := beta y_i + sum_j A(i, j) (alpha x_j), atomics in any order: K = entries of the row, R = 3 (alpha x_j, the product,
    beta y); beta == 0: y not read, R = 2"""
    col = np.repeat(np.arange(mat.n, dtype=np.int64), np.diff(mat.cp))
    t = mat.vx.astype(D) * (D(alpha) * x.astype(D))[col]
    acc = np.zeros(mat.m, dtype=D)
    ta = np.zeros(mat.m, dtype=D)
    np.add.at(acc, mat.ri, t)
    np.add.at(ta, mat.ri, abs(t))
    K = np.bincount(mat.ri, minlength=mat.m)
    if beta == 0:
        return Out(acc, ta, K, 2)
    by = D(beta) * y.astype(D)
    return Out(by + acc, abs(by) + ta, K, 3)


GEMV_M = [1, 255, 256, 257, 513]
GEMV_N = [0, 1, 2, 3, 4, 5, 7, 8, 9]


def c_dense_gemv(D, A, x, alpha, beta, y):
    """y := alpha A x + beta y, A m x n: four partial sums by column index mod 4 (the tail in the first), then two additions:
    K = n terms (the products are fused into the sums), R = 2 (beta y, then fma(alpha, r, .)); beta == 0: alpha r, R = 1"""
    A, x = A.astype(D), x.astype(D)
    r = A @ x if A.shape[1] else np.zeros(A.shape[0], dtype=D)
    tr = abs(A) @ abs(x) if A.shape[1] else np.zeros(A.shape[0], dtype=D)
    if beta == 0:
        return Out(D(alpha) * r, abs(D(alpha)) * tr, A.shape[1], 1)
    by = D(beta) * y.astype(D)
    return Out(D(alpha) * r + by, abs(D(alpha)) * tr + abs(by), A.shape[1], 2)


PACK_P = [1, 2, 255, 256, 257, 513]


# ---- 4. assembly S = G' diag(w) G (+ P) -----------------------------------------------------------------------------------------
ATDA_LENGTHS = [0, 1, 2, 3, 4, 5, 8, 9]            # and one of at least 64

Atda = collections.namedtuple("Atda", "name ml n Gp Gi Gx w Pp Pi Px")


def _from_dense_pattern(rng, B):
    ml, n = B.shape
    Gi = [np.flatnonzero(B[:, j]) for j in range(n)]
    Gp = np.concatenate([[0], np.cumsum([len(c) for c in Gi])]).astype(np.int64)
    Gi = np.concatenate(Gi).astype(np.int64) if Gp[-1] else np.zeros(0, dtype=np.int64)
    return Gp, Gi, spread(rng, Gp[-1])


def _lower_ccs(rng, n, pos):
    """CCS arrays of the entries pos = [(i, j), ...] in the order given within a column"""
    Pp = np.zeros(n + 1, dtype=np.int64)
    for _, j in pos:
        Pp[j + 1] += 1
    np.cumsum(Pp, out=Pp)
    Pi = np.array([i for j0 in range(n) for (i, j) in pos if j == j0], dtype=np.int64)
    return Pp, Pi, spread(rng, len(pos))


def pairs_pattern(dense_row):
    """G whose column pairs (2k, 2k + 1) share exactly (0, 1, 2, 3, 4, 7, 8, 70)[k] private rows [+ 1 with the dense row]; the last
    column and the last row are empty"""
    shared = [0, 1, 2, 3, 4, 7, 8, 70] if dense_row else [1, 2, 3, 4, 5, 8, 9, 70]
    n = 2 * len(shared) + 1
    ml = sum(shared) + (1 if dense_row else 0) + 1
    B = np.zeros((ml, n), dtype=bool)
    r = 0
    for k, s in enumerate(shared):
        B[r:r + s, 2 * k] = B[r:r + s, 2 * k + 1] = True
        r += s
    if dense_row:
        B[r, :n - 1] = True
    return B


def atda_cases(seed=43):
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, B, P):
        ml, n = B.shape
        Gp, Gi, Gx = _from_dense_pattern(rng, B)
        w = spread(rng, ml, signed=False)
        if P is None:
            Pp = Pi = Px = None
        else:
            Pp, Pi, Px = _lower_ccs(rng, n, P)
        cases.append(Atda(name, ml, n, Gp, Gi, Gx, w, Pp, Pi, Px))

    for dense_row in (False, True):
        B = pairs_pattern(dense_row)
        n = B.shape[1]
        tag = "dense_row" if dense_row else "pairs"
        diag = [(j, j) for j in range(n)]
        # a lower triangle: the diagonal (the empty column's entry is one that only P brings), entries on the pattern of G'G and
        # entries beside it
        lower = diag + [(1, 0), (2, 0), (5, 2), (n - 1, 0), (n - 1, n - 2), (3, 2), (6, 1)]
        add(tag, B, None)
        add(tag + "_Pdiag", B, diag)
        add(tag + "_Plower", B, lower)
    # snz = 1, 63, 64, 65: one entry per column in rows of its own (ml = 1 for snz = 1), with and without a diagonal P
    for snz in (1, 63, 64, 65):
        B = np.eye(snz, dtype=bool)
        add("snz%d" % snz, B, None)
        add("snz%d_Pdiag" % snz, B, [(j, j) for j in range(snz)])
    # ml = 1 with several columns: one dense row, every product list has one entry
    add("ml1", np.ones((1, 5), dtype=bool), [(j, j) for j in range(5)] + [(4, 0)])
    return cases


def dense_of(ml, n, cp, ri, vx, D):
    A = np.zeros((ml, n), dtype=D)
    col = np.repeat(np.arange(n), np.diff(cp))
    np.add.at(A, (ri, col), vx.astype(D))
    return A


def atda_pattern(case):
    """(Sp, Si, list length per entry): tril(G'G) united with tril(P), rows ascending"""
    B = dense_of(case.ml, case.n, case.Gp, case.Gi, np.ones(len(case.Gi)), F8) != 0
    cnt = B.T.astype(np.int64) @ B.astype(np.int64)
    M = cnt > 0
    if case.Pp is not None:
        pc = np.repeat(np.arange(case.n), np.diff(case.Pp))
        low = case.Pi >= pc
        M[case.Pi[low], pc[low]] = True
    M = np.tril(M)
    Si = [np.flatnonzero(M[:, j]) for j in range(case.n)]
    Sp = np.concatenate([[0], np.cumsum([len(c) for c in Si])]).astype(np.int64)
    Si = np.concatenate(Si).astype(np.int64) if Sp[-1] else np.zeros(0, dtype=np.int64)
    sc = np.repeat(np.arange(case.n), np.diff(Sp))
    return Sp, Si, cnt[Si, sc]


def a_assemble(D, case, sq=False, Px=None, Pp=None, Pi=None):
    """S_ij = sum_r (w_r G_ri) G_rj (+ the entries of P at (i, j), i >= j, in the order stored): K = products + entries of P,
    R = 2 (w G, then its product with G) [+ 1: w = di^2].  An entry without products is the entry of P, exactly."""
    Pp = case.Pp if Pp is None else Pp
    Pi = case.Pi if Pi is None else Pi
    Px = case.Px if Px is None else Px
    G = dense_of(case.ml, case.n, case.Gp, case.Gi, case.Gx, D)
    w = case.w.astype(D)
    if sq:
        w = w * w
    S = G.T @ (w[:, None] * G)
    T = abs(G).T @ (abs(w)[:, None] * abs(G))
    Sp, Si, lens = atda_pattern(case._replace(Pp=Pp, Pi=Pi, Px=Px))
    K = lens.astype(np.int64).copy()
    sc = np.repeat(np.arange(case.n), np.diff(Sp))
    ref, tt = S[Si, sc].copy(), T[Si, sc].copy()
    if Pp is not None:
        slot = {(int(i), int(j)): e for e, (i, j) in enumerate(zip(Si, sc))}
        pc = np.repeat(np.arange(case.n), np.diff(Pp))
        for q in range(len(Pi)):
            if Pi[q] >= pc[q]:
                e = slot[(int(Pi[q]), int(pc[q]))]
                ref[e] = ref[e] + D(Px[q])
                tt[e] = tt[e] + abs(D(Px[q]))
                K[e] += 1
    return Out(ref, tt, K, 3 if sq else 2), lens


# ---- 5. fused kernels -------------------------------------------------------------------------------------------------------
FUSED_LONGEST = [1, 4, 5, 8, 9, 16, 17, 33]


def lanes_for(longest):
    return 4 if 0 < longest <= 4 else (8 if 0 < longest <= 8 else 16)


def residual_lanes(max_col, max_row):
    return (16 if lanes_for(max_col) == 16 else 8, 4 if lanes_for(max_row) == 4 else 16)


def groups16(rows, lanes=16):
    return min(max((rows * lanes + 255) // 256, 1), CAP_GROUPS)


def fused_block(rng, lc, lr, rep=5):
    """G of rep diagonal blocks, each (lc + 2) x (lr + 2): column 0 holds rows 0 .. lc - 1, row lc holds columns 1 .. lr, the last
    row and the last column are empty: the longest column has lc entries, the longest row lr"""
    bm, bn = lc + 2, lr + 2
    B = np.zeros((rep * bm, rep * bn), dtype=bool)
    for b in range(rep):
        B[b * bm:b * bm + lc, b * bn] = True
        B[b * bm + lc, b * bn + 1:b * bn + 1 + lr] = True
    Gp, Gi, Gx = _from_dense_pattern(rng, B)
    return Mat("c%d_r%d" % (lc, lr), B.shape[0], B.shape[1], Gp, Gi, Gx)


def fused_mats(seed=47):
    rng = np.random.default_rng(seed)
    mats = [fused_block(rng, L, L) for L in FUSED_LONGEST]
    mats += [fused_block(rng, 17, 4), fused_block(rng, 4, 17)]          # the (16, 4) and (8, 16) residual kernels
    return mats


def circulant(rng, ml, n, name):
    """row i holds columns i mod n and (i + 1) mod n (one entry where they coincide: n = 1)"""
    i = np.arange(ml, dtype=np.int64)
    rows = np.concatenate([i, i]) if n > 1 else i
    cols = np.concatenate([i % n, (i + 1) % n]) if n > 1 else i % n
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=cp[1:])
    return Mat(name, ml, n, cp, np.ascontiguousarray(rows), spread(rng, len(rows)))


def fused_big_mats(seed=53):
    """past the caps with hint 0 (16 lanes): 262145 rows and columns are one group more than 16384 workgroups hold (post, pre,
    residuals); 1048577 columns are one workgroup more than the 4096 of post's x part"""
    rng = np.random.default_rng(seed)
    return [circulant(rng, 262145, 262145, "sq262145"), circulant(rng, 257, 1048577, "wide1048577")]


def f_pre(D, mat, di, xs, xin, zin):
    """x2_j := xs xin_j + sum_i G_ij (di_i (zin_i di_i)): K = entries of the column, R = 4 (z di, di (.), xs xin, the last addition;
    the product of a term is fused into the sum)"""
    di, zin = di.astype(D), zin.astype(D)
    t = mat.vx.astype(D) * (di * (zin * di))[mat.ri]
    x0 = D(xs) * xin.astype(D)
    return Out(x0 + gather_sum(D, mat.n, mat.cp, t), abs(x0) + gather_sum(D, mat.n, mat.cp, abs(t)), np.diff(mat.cp), 4)


def f_post(D, mat, tmat, di, xos, zos, zin, x2):
    """xout := xos x2 (R 1); zout_i := zos (di_i (G x2)_i - zin_i di_i): K = entries of the row, R = 4.  tmat: the transpose's CCS"""
    tp, ti, tx = tmat
    di, x2 = di.astype(D), x2.astype(D)
    t = tx.astype(D) * x2[ti]
    acc, ta = gather_sum(D, mat.m, tp, t), gather_sum(D, mat.m, tp, abs(t))
    zs = zin.astype(D) * di
    xo = x2 * D(xos)
    return dict(xout=Out(xo, abs(xo), 0, 1),
                zout=Out((di * acc - zs) * D(zos), (abs(di) * ta + abs(zs)) * abs(D(zos)), np.diff(tp), 4))


def f_residuals(D, mat, tmat, x, z, s, c, h, tau):
    """hrx := -G'z (K = column entries, R = 0); rx := hrx - tau c (R 1); hrz := G x + s (K = row entries, R 1); rz := hrz - tau h (R 2)"""
    tp, ti, tx = tmat
    t = mat.vx.astype(D) * z.astype(D)[mat.ri]
    a, ta = gather_sum(D, mat.n, mat.cp, t), gather_sum(D, mat.n, mat.cp, abs(t))
    u = tx.astype(D) * x.astype(D)[ti]
    b, tb = gather_sum(D, mat.m, tp, u), gather_sum(D, mat.m, tp, abs(u))
    tc, th = D(tau) * c.astype(D), D(tau) * h.astype(D)
    kc, kr = np.diff(mat.cp), np.diff(tp)
    hrz, thz = b + s.astype(D), tb + abs(s.astype(D))
    return dict(hrx=Out(-a, ta, kc, 0), rx=Out(-a - tc, ta + abs(tc), kc, 1), hrz=Out(hrz, thz, kr, 1), rz=Out(hrz - th, thz + abs(th), kr, 2))


HALF_ML = [1, 255, 256, 257, 65537]
HALF_N = [1, 524289]
HALF_P = [0, 1, 300]


def half_cases():
    """(ml, n, p, z1'z1 given by the host, ws3 given): every ml with both n, every p and both values of either switch"""
    return [(1, 1, 0, False, True), (1, 524289, 1, True, False), (255, 1, 300, False, False), (255, 524289, 0, True, True),
            (256, 1, 1, True, True), (256, 524289, 300, False, True), (257, 524289, 0, False, False), (257, 1, 300, True, False),
            (65537, 524289, 1, False, True), (65537, 1, 0, True, False)]


def half_data(ml, n, p, seed=59):
    rng = np.random.default_rng(seed + 7 * ml + 3 * n + p)
    v = dict(c=spread(rng, n), dx=spread(rng, n), x1=spread(rng, n), th=spread(rng, ml), dz=spread(rng, ml), z1=spread(rng, ml),
             ds=spread(rng, ml), lm=spread(rng, ml, signed=False), b=spread(rng, max(p, 1)), dy=spread(rng, max(p, 1)),
             y1=spread(rng, max(p, 1)), dgi=0.84375, dtau0=-1.3125)
    return v


def h_dtau(D, v, ml, n, p, z1z1):
    """dtau = dgi (dtau0 + c'dx + b'dy + th'dz) / (1 + z1'z1): the three (two: p = 0) inner products on the fixed tree, K = the
    deepest of them plus the tree of z1'z1 (0 where the host gives it); R = 8: the product inside the trees of the numerator (1)
    and of z1'z1 (1), three additions, 1 + zz, the product with dgi, the division.  Returns (dtau, z1'z1)."""
    r0 = r_dot(D, v["c"], v["dx"])
    r2 = r_dot(D, v["th"], v["dz"])
    K = max(r0.K, r2.K)
    num, tn = D(v["dtau0"]) + r0.ref[0] + r2.ref[0], abs(D(v["dtau0"])) + r0.T[0] + r2.T[0]
    if p > 0:
        r1 = r_dot(D, v["b"][:p], v["dy"][:p])
        num, tn, K = num + r1.ref[0], tn + r1.T[0], max(K, r1.K)
    if z1z1 is None:
        r3 = r_dot(D, v["z1"], v["z1"])
        zz, kz = r3.ref[0], r3.K
        zout = Out(r3.ref, r3.T, r3.K, 1)
    else:
        zz, kz = D(z1z1), 0
        zout = None
    val = D(v["dgi"]) * num / (1 + zz)
    return Out(np.array([val]), np.array([abs(D(v["dgi"])) * tn / (1 + zz)]), K + kz, 8), zout


# ---- coverage ---------------------------------------------------------------------------------------------------------------
def coverage():
    """the edges the case lists reach, as sets and flags (test_kkt_edges_cpu.py names those that must be there)"""
    cov = {}
    cov["elem_mod256"] = {n % 256 for n in ELEM_SIZES}
    cov["elem_over_cap"] = {n > CAP_GRID * 256 for n in ELEM_SIZES}
    cov["red_mod256"] = {n % 256 for n in RED_SIZES}
    cov["red_per"] = {red_per(n) for n in RED_SIZES}
    cov["red_second_trip"] = {red_per(n) > 256 for n in RED_SIZES}
    cov["plants"] = set().union(*[set(max_step_plants(n)) for n in RED_SIZES])
    cov["multi_counts"] = {len(s) for _, s in multi_cases()}
    cov["multi_mixed"] = any({k for k, _ in s} == {0, 1} for _, s in multi_cases())
    cov["multi_empty_sum"] = any((0, 0) in s for _, s in multi_cases())
    tm = spmv_t_mats()
    cov["spmv_t_lens"] = set().union(*[set(np.diff(a.cp).tolist()) for a in tm])
    cov["spmv_t_n"] = {a.n for a in tm}
    cov["spmv_t_empty_ends"] = all(a.cp[1] == 0 and a.cp[-1] == a.cp[-2] for a in tm if a.n > 1)
    cov["spmv_t_over_cap"] = {a.n * 16 > CAP_GRID * 256 for a in tm}
    nm = spmv_n_mats()
    cov["spmv_n_rowlens"] = set().union(*[set(np.bincount(a.ri, minlength=a.m).tolist()) for a in nm])
    cov["spmv_n_over_cap"] = {a.n > CAP_GRID * 256 for a in nm}
    sm = spmm_mat()
    cov["spmm_over_cap"] = sm.n * 16 > CAP_SPMM * 256
    cov["spmm_lens"] = set(np.diff(sm.cp).tolist())
    cov["gemv_m_mod256"] = {m % 256 for m in GEMV_M}
    cov["gemv_blocks"] = {(m + 255) // 256 for m in GEMV_M}
    cov["gemv_n_mod4"] = {(n // 4 > 0, n % 4) for n in GEMV_N}
    cov["pack_blocks"] = {(p + 255) // 256 for p in PACK_P}
    cov["pack_mod256"] = {p % 256 for p in PACK_P}
    lens, snz4, flags = set(), set(), set()
    for c in atda_cases():
        Sp, Si, ln = atda_pattern(c)
        lens |= set(int(v) for v in ln)
        snz4.add(((4 * len(Si)) // 256, (4 * len(Si)) % 256) if len(Si) in (1, 63, 64, 65) else None)
        rows = np.bincount(c.Gi, minlength=c.ml)
        if rows.max() >= c.n - 1 and c.n > 2:
            flags.add("dense_row")
        if rows.min() == 0:
            flags.add("empty_row")
        if np.diff(c.Gp).min() == 0:
            flags.add("empty_col")
        if c.ml == 1:
            flags.add("ml1")
        flags.add("P" if c.Pp is not None else "noP")
        if c.Pp is not None:
            pc = np.repeat(np.arange(c.n), np.diff(c.Pp))
            flags.add("Pdiag" if np.all(c.Pi == pc) else "Plower")
    cov["atda_lens"] = lens
    cov["atda_4snz_mod256"] = snz4 - {None}
    cov["atda_snz"] = {len(atda_pattern(c)[1]) for c in atda_cases()}
    cov["atda_flags"] = flags
    fm = fused_mats()
    cov["fused_max_col"] = {int(np.diff(a.cp).max()) for a in fm}
    cov["fused_max_row"] = {int(np.bincount(a.ri, minlength=a.m).max()) for a in fm}
    cov["fused_empty"] = all(np.diff(a.cp).min() == 0 and np.bincount(a.ri, minlength=a.m).min() == 0 for a in fm)
    cov["fused_lanes_col"] = {lanes_for(int(np.diff(a.cp).max())) for a in fm}
    cov["fused_lanes_row"] = {lanes_for(int(np.bincount(a.ri, minlength=a.m).max())) for a in fm}
    cov["fused_residual_kernels"] = {residual_lanes(int(np.diff(a.cp).max()), int(np.bincount(a.ri, minlength=a.m).max())) for a in fm}
    big = fused_big_mats()
    cov["fused_rows_over_cap"] = any((a.m * 16 + 255) // 256 > CAP_GROUPS for a in big)
    cov["fused_cols_over_cap"] = any((a.n * 16 + 255) // 256 > CAP_GROUPS for a in big)
    cov["fused_post_x_over_cap"] = any((a.n + 255) // 256 > CAP_POST_X for a in big)
    hc = half_cases()
    cov["half_ml"] = {c[0] for c in hc}
    cov["half_n"] = {c[1] for c in hc}
    cov["half_p"] = {c[2] for c in hc}
    cov["half_host_zz"] = {c[3] for c in hc}
    cov["half_ws3"] = {c[4] for c in hc}
    cov["half_x_over_cap"] = any((max(c[1], c[2]) + 255) // 256 > CAP_GRID for c in hc)
    return cov
