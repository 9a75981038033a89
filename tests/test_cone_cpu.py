"""kvx_cone_plan (csrc/cone_api.cpp): the pattern of S = Gs' Gs for 'l', 'q' and 's' blocks is the union of the cliques of
columns that touch each row / cone / lower triangle of a block -- host only, no GPU."""
import ctypes

import numpy as np
import pytest

from kvxopt_amd import _lib


def _plan(ml, q, s, n, G):
    """G: dense N x n numpy array -> (snz, Sp, Si) of kvx_cone_plan on its nonzero pattern."""
    N = G.shape[0]
    cols = [np.nonzero(G[:, j])[0] for j in range(n)]
    Gp = np.zeros(n + 1, dtype=np.int64)
    Gp[1:] = np.cumsum([c.size for c in cols])
    Gi = np.concatenate(cols).astype(np.int64) if Gp[-1] else np.zeros(1, dtype=np.int64)
    qa = np.asarray(q, dtype=np.int64)
    sa = np.asarray(s, dtype=np.int64)
    h = ctypes.c_void_p()
    L = _lib.lib()
    rc = L.kvx_cone_plan(ml, len(q), _lib.pi(qa) if q else None, len(s), _lib.pi(sa) if s else None, n, _lib.pi(Gp), _lib.pi(Gi),
                         ctypes.byref(h))
    assert rc == 0, _lib.last_error()
    try:
        snz = ctypes.c_int64()
        assert L.kvx_cone_pattern(h, ctypes.byref(snz), None, None) == 0
        Sp = np.zeros(n + 1, dtype=np.int64)
        Si = np.zeros(max(snz.value, 1), dtype=np.int64)
        assert L.kvx_cone_pattern(h, ctypes.byref(snz), _lib.pi(Sp), _lib.pi(Si)) == 0
    finally:
        L.kvx_cone_free(h)
    return Sp, Si[:snz.value]


def _expected(ml, q, s, n, G):
    """numpy: the lower pattern of the union of the cliques."""
    P = np.zeros((n, n), dtype=bool)
    B = [np.arange(r, r + 1) for r in range(ml)]
    r = ml
    for k in q:
        B.append(np.arange(r, r + k)); r += k
    for m in s:
        rows = [r + i + m * j for j in range(m) for i in range(j, m)]     # lower triangle only
        B.append(np.asarray(rows, dtype=np.int64)); r += m * m
    for rows in B:
        C = np.nonzero(np.any(G[rows, :] != 0, axis=0))[0] if rows.size else np.zeros(0, int)
        P[np.ix_(C, C)] = True
    return np.tril(P)


def _to_dense(n, Sp, Si):
    P = np.zeros((n, n), dtype=bool)
    for j in range(n):
        P[Si[Sp[j]:Sp[j + 1]], j] = True
    return P


@pytest.mark.parametrize("case", [
    (3, [4, 4], [3], 3, 0.6, 1),          # the shape of the reference's conelp example
    (0, [], [5, 2], 12, 0.15, 2),         # 's' only
    (5, [3, 1, 6], [], 20, 0.1, 3),       # 'q' only, a cone of order 1
    (4, [2], [0, 4, 0], 9, 0.3, 4),       # 's' blocks of order 0
    (0, [7], [6], 30, 0.04, 5),           # columns touched by no block
])
def test_pattern_is_the_union_of_the_cliques(case):
    ml, q, s, n, dens, seed = case
    rng = np.random.default_rng(seed)
    N = ml + sum(q) + sum(m * m for m in s)
    G = rng.standard_normal((N, n)) * (rng.random((N, n)) < dens)
    Sp, Si = _plan(ml, q, s, n, G)
    assert np.all(np.diff(Sp) >= 0) and Sp[-1] == Si.size
    for j in range(n):
        col = Si[Sp[j]:Sp[j + 1]]
        assert np.all(np.diff(col) > 0) and (col.size == 0 or col[0] >= j)
    np.testing.assert_array_equal(_to_dense(n, Sp, Si), _expected(ml, q, s, n, G))


def test_strict_upper_triangle_of_an_s_block_does_not_enter_the_pattern():
    # one 3 x 3 block; column 0 has a nonzero only in the strict upper triangle (row 0 + 3 * 2 = entry (0, 2)), column 1 only
    # on the diagonal, column 2 in the lower triangle: S couples 1 and 2 only
    n, m = 3, 3
    G = np.zeros((m * m, n))
    G[0 + m * 2, 0] = 1.0
    G[1 + m * 1, 1] = 2.0
    G[2 + m * 0, 2] = 3.0
    Sp, Si = _plan(0, [], [m], n, G)
    P = _to_dense(n, Sp, Si)
    assert not P[:, 0].any() and not P[0, :].any()
    assert P[1, 1] and P[2, 2] and P[2, 1]


def test_argument_errors_are_library_codes():
    L = _lib.lib()
    h = ctypes.c_void_p()
    Gp = np.zeros(3, dtype=np.int64)
    Gi = np.zeros(1, dtype=np.int64)
    bad_q = np.array([0], dtype=np.int64)
    assert L.kvx_cone_plan(0, 1, _lib.pi(bad_q), 0, None, 2, _lib.pi(Gp), _lib.pi(Gi), ctypes.byref(h)) == _lib.KVX_EINVAL
    bad_s = np.array([-1], dtype=np.int64)
    assert L.kvx_cone_plan(0, 0, None, 1, _lib.pi(bad_s), 2, _lib.pi(Gp), _lib.pi(Gi), ctypes.byref(h)) == _lib.KVX_EINVAL
    Gp2 = np.array([0, 1, 1], dtype=np.int64)
    Gi2 = np.array([5], dtype=np.int64)                          # row 5 of a 2-row G
    assert L.kvx_cone_plan(2, 0, None, 0, None, 2, _lib.pi(Gp2), _lib.pi(Gi2), ctypes.byref(h)) == _lib.KVX_EINVAL
    assert L.kvx_cone_plan(-1, 0, None, 0, None, 2, _lib.pi(Gp), _lib.pi(Gi), ctypes.byref(h)) == _lib.KVX_EINVAL
    assert L.kvx_cone_pattern(None, None, None, None) == _lib.KVX_EINVAL
    assert L.kvx_cone_assemble_dev(None, None, None, None, None, None, None) == _lib.KVX_EINVAL
