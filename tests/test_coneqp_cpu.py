"""kvx_cone_plan_h (csrc/cone_api.cpp): the pattern of S = H + Gs' Gs is the union of the cliques of G and the lower triangle of
H; without an H pattern it is the pattern of kvx_cone_plan -- host only, no GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

from kvxopt_amd import _lib

_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_G21 = json.load(open(os.path.join(_GOLD, "g21_coneqp_cones.json")))


def _ccs_pattern(M):
    """Nonzero pattern of a dense array as CCS (colptr, rowind)."""
    n = M.shape[1]
    cols = [np.nonzero(M[:, j])[0] for j in range(n)]
    cp = np.zeros(n + 1, dtype=np.int64)
    cp[1:] = np.cumsum([c.size for c in cols])
    ri = np.concatenate(cols).astype(np.int64) if cp[-1] else np.zeros(1, dtype=np.int64)
    return cp, ri


def _pattern_of(h, n):
    L = _lib.lib()
    try:
        snz = ctypes.c_int64()
        assert L.kvx_cone_pattern(h, ctypes.byref(snz), None, None) == 0
        Sp = np.zeros(n + 1, dtype=np.int64)
        Si = np.zeros(max(snz.value, 1), dtype=np.int64)
        assert L.kvx_cone_pattern(h, ctypes.byref(snz), _lib.pi(Sp), _lib.pi(Si)) == 0
    finally:
        L.kvx_cone_free(h)
    P = np.zeros((n, n), dtype=bool)
    for j in range(n):
        col = Si[Sp[j]:Sp[j + 1]]
        assert np.all(np.diff(col) > 0) and (col.size == 0 or col[0] >= j)
        P[col, j] = True
    assert Sp[-1] == snz.value
    return P


def _plan_h(ml, q, s, n, G, H):
    """Dense G (N x n) and H (n x n, or None): the pattern of kvx_cone_plan_h as a dense boolean array."""
    Gp, Gi = _ccs_pattern(G)
    qa, sa = np.asarray(q, dtype=np.int64), np.asarray(s, dtype=np.int64)
    h = ctypes.c_void_p()
    Hp = Hi = None
    if H is not None:
        Hp, Hi = _ccs_pattern(H)
    rc = _lib.lib().kvx_cone_plan_h(ml, len(q), _lib.pi(qa) if q else None, len(s), _lib.pi(sa) if s else None, n, _lib.pi(Gp),
                                    _lib.pi(Gi), _lib.pi(Hp) if H is not None else None, _lib.pi(Hi) if H is not None else None,
                                    ctypes.byref(h))
    assert rc == 0, _lib.last_error()
    return _pattern_of(h, n)


def _plan(ml, q, s, n, G):
    Gp, Gi = _ccs_pattern(G)
    qa, sa = np.asarray(q, dtype=np.int64), np.asarray(s, dtype=np.int64)
    h = ctypes.c_void_p()
    rc = _lib.lib().kvx_cone_plan(ml, len(q), _lib.pi(qa) if q else None, len(s), _lib.pi(sa) if s else None, n, _lib.pi(Gp),
                                  _lib.pi(Gi), ctypes.byref(h))
    assert rc == 0, _lib.last_error()
    return _pattern_of(h, n)


def _cliques(ml, q, s, n, G):
    """numpy: the lower pattern of the union of the cliques of the 'l' rows, 'q' cones and lower triangles of the 's' blocks."""
    P = np.zeros((n, n), dtype=bool)
    B = [np.arange(r, r + 1) for r in range(ml)]
    r = ml
    for k in q:
        B.append(np.arange(r, r + k)); r += k
    for m in s:
        B.append(np.asarray([r + i + m * j for j in range(m) for i in range(j, m)], dtype=np.int64)); r += m * m
    for rows in B:
        C = np.nonzero(np.any(G[rows, :] != 0, axis=0))[0] if rows.size else np.zeros(0, int)
        P[np.ix_(C, C)] = True
    return np.tril(P)


def _g21(name):
    Z = np.load(os.path.join(_GOLD, "g21_coneqp_cones.npz"))
    d = _G21["cases"][name]["dims"]
    return Z[name + "__G"], Z[name + "__P"], d["l"], list(d["q"]), list(d["s"])


@pytest.mark.parametrize("name", ["p_zero", "p_widens_pattern", "p_upper_garbage"])
def test_pattern_is_the_union_of_the_cliques_and_the_lower_triangle_of_h(name):
    G, P, ml, q, s = _g21(name)
    n = G.shape[1]
    cl = _cliques(ml, q, s, n, G)
    want = cl | np.tril(P != 0)
    got = _plan_h(ml, q, s, n, G, P)                    # P with whatever lies above its diagonal: ignored
    np.testing.assert_array_equal(got, want)
    if name == "p_zero":
        assert not (P != 0).any()
        np.testing.assert_array_equal(got, cl)
    if name == "p_widens_pattern":
        assert (want & ~cl).any()                       # the case is what its name says
    if name == "p_upper_garbage":
        assert (np.triu(P, 1) != 0).any() and not np.array_equal(np.triu(P, 1), np.tril(P, -1).T)
        np.testing.assert_array_equal(got, _plan_h(ml, q, s, n, G, np.tril(P)))


@pytest.mark.parametrize("case", [
    (3, [4, 4], [3], 3, 0.6, 1),
    (0, [], [5, 2], 12, 0.15, 2),
    (5, [3, 1, 6], [], 20, 0.1, 3),
    (0, [7], [6], 30, 0.04, 5),
])
def test_without_an_h_pattern_it_is_the_plan_of_today(case):
    ml, q, s, n, dens, seed = case
    rng = np.random.default_rng(seed)
    N = ml + sum(q) + sum(m * m for m in s)
    G = rng.standard_normal((N, n)) * (rng.random((N, n)) < dens)
    base = _plan(ml, q, s, n, G)
    np.testing.assert_array_equal(_plan_h(ml, q, s, n, G, None), base)
    np.testing.assert_array_equal(base, _cliques(ml, q, s, n, G))
    # an H that holds nothing: the same pattern again
    np.testing.assert_array_equal(_plan_h(ml, q, s, n, G, np.zeros((n, n))), base)
    # a random H: the union
    H = rng.standard_normal((n, n)) * (rng.random((n, n)) < 0.1)
    np.testing.assert_array_equal(_plan_h(ml, q, s, n, G, H), base | np.tril(H != 0))


def test_h_alone_gives_its_lower_triangle():
    # no rows in G at all: S = H
    n = 6
    H = np.zeros((n, n))
    H[[0, 3, 5, 5], [0, 1, 2, 5]] = 1.0
    H[1, 4] = 7.0                                       # above the diagonal
    got = _plan_h(0, [], [], n, np.zeros((0, n)), H)
    np.testing.assert_array_equal(got, np.tril(H != 0))


def test_argument_errors_are_library_codes():
    L = _lib.lib()
    h = ctypes.c_void_p()
    Gp = np.zeros(3, dtype=np.int64)
    Gi = np.zeros(1, dtype=np.int64)
    ok_p = np.array([0, 1, 2], dtype=np.int64)
    ok_i = np.array([0, 1], dtype=np.int64)
    plan = lambda Hp, Hi, n=2, ml=0: L.kvx_cone_plan_h(ml, 0, None, 0, None, n, _lib.pi(Gp), _lib.pi(Gi), _lib.pi(Hp),
                                                       _lib.pi(Hi) if Hi is not None else None, ctypes.byref(h))
    assert plan(ok_p, ok_i) == _lib.KVX_OK
    L.kvx_cone_free(h)
    assert plan(np.array([0, 1, 2], dtype=np.int64), np.array([0, 2], dtype=np.int64)) == _lib.KVX_EINVAL      # row 2 of a 2 x 2 H
    assert plan(np.array([0, 1, 2], dtype=np.int64), np.array([-1, 1], dtype=np.int64)) == _lib.KVX_EINVAL
    assert plan(np.array([0, 2, 1], dtype=np.int64), ok_i) == _lib.KVX_EINVAL                                   # colptr decreases
    assert plan(np.array([1, 1, 2], dtype=np.int64), ok_i) == _lib.KVX_EINVAL                                   # colptr[0] != 0
    assert plan(ok_p, None) == _lib.KVX_EINVAL                                                                  # entries without rows
    assert plan(np.array([0, 2, 2], dtype=np.int64), np.array([1, 1], dtype=np.int64)) == _lib.KVX_EINVAL      # an entry twice
    assert b"twice" in L.kvx_last_error()
    assert plan(ok_p, ok_i, ml=-1) == _lib.KVX_EINVAL
    assert L.kvx_cone_plan_h(0, 0, None, 0, None, 2, _lib.pi(Gp), _lib.pi(Gi), _lib.pi(ok_p), _lib.pi(ok_i), None) == _lib.KVX_EINVAL
    assert L.kvx_cone_assemble_h_dev(None, None, None, None, None, None, None, None) == _lib.KVX_EINVAL
    # values of H on a plan that has no H pattern
    assert L.kvx_cone_plan(0, 0, None, 0, None, 2, _lib.pi(Gp), _lib.pi(Gi), ctypes.byref(h)) == _lib.KVX_OK
    dummy = ctypes.c_void_p(8)
    assert L.kvx_cone_assemble_h_dev(h, None, None, None, None, None, dummy, dummy) == _lib.KVX_EINVAL
    L.kvx_cone_free(h)
