"""Child process of the trailing-update schedule tests (test_syrk_schedules_gpu.py, test_chol_gpu.py::test_syrk128_variant_parity).

The schedule knobs of the big fronts' pivot chain (KVX_DEFER_U, KVX_SYRK_DIRECT, KVX_PAIR_TILES, KVX_BLOCKED_GF, KVX_U_STREAM,
KVX_SYRK_LDS_TILES, KVX_FAR_WGS) are read once per factor or once per process (chol_internal.hpp CholKnobs), so every setting runs in a process of its own.  For each matrix named
on the command line the child factors three times -- eagerly, under capture, from the replayed graph -- and checks the factor
entries, diag() and the solves of sys 0-8 against the CPU oracle (prepared once by the parent: `prepare`), the residual, the bits
of the three factorisations, and reports the trailing-update launches per kernel (kvx_dbg_syrk_counts) as one RESULT line.

Also imported by the tests for the matrices and for the chain lists of a factor (rebuilt from the analysis, as chol_setup.cpp
build_chain_lists does)."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INT_MAX = 2**31 - 1
NB = 64
COUNTERS = ["t64_cls", "t64_grid", "t128_cls", "t128_grid", "lds", "lds_far", "lds_far_stride", "t128_panel", "outer", "far_side"]
# no relaxed amalgamation: a gadget's fronts are its fundamental supernodes
GADGET_OPTS = {"relax_small": 0, "relax_z1": 0.0, "relax_z2": 0.0, "relax_z3": 0.0, "leaf_cols": 0}
# (m, k) of the big fronts of one level: the lists whose tile classes overlapped before the class-bounded decode
GADGETS = {
    "gadget_near512": [(2100, 812), (1500, 1100)],     # near launch of KVX_U_BLOCK=512: rectangular class, then triangular T = 16
    "gadget_pair0": [(1020, 127), (1019, 1)],          # pair launch at kb = 0: T 14 -> 16
    "gadget_pair256": [(1276, 383), (1275, 257)],      # pair launch at kb = 256
}


def gadget(fronts, seed=0):
    """SPD matrix (lower CCS, natural order) whose level-1 big fronts are exactly `fronts` = [(m, k), ...]: per front an
    independent block of a dense child of k columns fully coupled to a dense parent of m - k columns, and one more column
    coupled to the parent alone (without it the child and the parent would be one supernode: the child's last column and the
    parent's first would have the same rows)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    blocks = []
    for m, k in fronts:
        nb = m + 1
        A = rng.uniform(-1.0, 1.0, (nb, nb))
        A = np.tril(A, -1)
        A[m, :k] = 0.0                                  # the last column is not coupled to the child
        A = A + A.T
        A[np.arange(nb), np.arange(nb)] = np.abs(A).sum(axis=1) + 1.0
        blocks.append(sp.csc_matrix(np.tril(A)))
    L = sp.block_diag(blocks, format="csc")
    L.sort_indices()
    return L.shape[0], L.indptr.astype(np.int64), L.indices.astype(np.int64), L.data.copy()


def random_spd(n, dens, seed, shift):
    import scipy.sparse as sp
    M = sp.random(n, n, dens, random_state=seed, format="csc")
    S = (M @ M.T + sp.eye(n) * shift).tocsc()
    L = sp.tril(S).tocsc(); L.sort_indices()
    return n, L.indptr.astype(np.int64), L.indices.astype(np.int64), L.data.copy()


def dense_rows(g, nd, seed=3):
    """2-D Laplacian with nd dense rows (and columns): fronts of few pivots with long update regions."""
    import scipy.sparse as sp
    from kvxopt_amd import workloads
    n0, cp, ri, v = workloads.laplacian_2d(g)
    rng = np.random.default_rng(seed)
    A = sp.csc_matrix((v, ri, cp), shape=(n0, n0))
    n = n0 + nd
    C = sp.csc_matrix(rng.uniform(-0.01, 0.01, (nd, n0)))
    D = sp.eye(nd) * (n0 * 0.01 + 10.0)
    full = sp.bmat([[A + sp.triu(A.T, 1), C.T], [C, D]]).tocsc()
    L = sp.tril(full).tocsc(); L.sort_indices()
    return n, L.indptr.astype(np.int64), L.indices.astype(np.int64), L.data.copy()


def matrix(name):
    """name -> (n, colptr, rowind, values, perm, opts)"""
    from kvxopt_amd import workloads
    if name in GADGETS:
        n, cp, ri, v = gadget(GADGETS[name])
        return n, cp, ri, v, np.arange(n), GADGET_OPTS
    if name == "rand2500":                                          # the matrix of the old test_syrk128_variant_parity
        return random_spd(2500, 0.02, 4, 5.0) + (None, None)
    if name == "lap150":
        return workloads.laplacian_2d(150) + (None, None)
    if name == "stencil21_40":
        return workloads.stencil21_2d(40) + (None, None)
    if name == "dense_rows":
        return dense_rows(70, 6) + (None, None)
    raise KeyError(name)


ALL_MATRICES = list(GADGETS) + ["rand2500", "lap150", "stencil21_40", "dense_rows"]


# ---- the chain lists of a factor (chol_setup.cpp build_chain_lists) ----------------------------------------------------------------
def front_class_big(m, k):
    return m > 128 or k > 64


def chain_levels(F):
    """per level with big fronts: (orders, pivot counts) of the big fronts in level-list order (symbolic.cpp: by level, big
    fronts first, largest order first, stable in supernode order)"""
    sup, nrows, _, level = F.supernodes()
    k = np.diff(sup)
    out = {}
    for s in range(len(nrows)):
        if front_class_big(int(nrows[s]), int(k[s])):
            out.setdefault(int(level[s]), []).append(s)
    res = {}
    for l, fs in out.items():
        fs = sorted(fs, key=lambda s: -int(nrows[s]))               # (sorted() is stable)
        res[l] = ([int(nrows[s]) for s in fs], [int(k[s]) for s in fs])
    return res


def chain_list(hm, hk, kb, far, u_block):
    """the fronts of one launch list, largest region first (build_chain_lists' emit)"""
    def region(i):
        return hm[i] - min(kb + 2 * u_block, hk[i]) if far else hm[i]
    act = [i for i in range(len(hm)) if hk[i] > kb and region(i) > 0]
    act.sort(key=lambda i: -region(i))
    return [hm[i] for i in act], [hk[i] for i in act]


def launch_shapes(hm, hk, u_block):
    """every (uonly, list m, list k, kb, klen, col_lim) launch the schedules issue over one level's big fronts"""
    maxk = max(hk)
    for jb in range(0, maxk, NB):
        m, k = chain_list(hm, hk, jb, False, u_block)
        ob = jb - jb % u_block
        yield (0, m, k, jb, NB, INT_MAX)                            # plain
        yield (0, m, k, jb, 2 * NB, INT_MAX)                        # pair: both panels
        yield (0, m, k, jb, NB, jb + 2 * NB)                        # pair: the second panel's columns
        yield (0, m, k, jb, NB, ob + u_block)                       # blocked: inner
        if jb == ob:
            yield (0, m, k, ob, u_block, ob + 2 * u_block)          # blocked: near
            fm, fk = chain_list(hm, hk, ob, True, u_block)
            yield (1, fm, fk, ob, u_block, ob + 2 * u_block)        # blocked: far


# ---- the parent's side: oracle results once per matrix ------------------------------------------------------------------------
def _rhs(n):
    return np.random.default_rng(n).standard_normal((n, 3))


def prepare(name, cache_dir):
    """CPU only: analysis (the permutation) and the oracle's factor, diag and solves, saved for the children"""
    from kvxopt_amd.chol import Factor
    from oracle.kvx_oracle import OracleChol
    n, cp, ri, v, perm, opts = matrix(name)
    F = Factor(n, cp, ri, "L", perm, opts)
    p = F.perm()
    O = OracleChol(n, cp, ri, "L", p)
    O.factorize(v)
    B = _rhs(n)
    X = []
    for s in range(9):
        Xo = np.asfortranarray(B.copy())
        O.solve(Xo, sys=s)
        X.append(Xo)
    Op, Oi, Ox = O.L()
    np.savez(os.path.join(cache_dir, name + ".npz"), perm=p, Op=Op, Oi=Oi, Ox=Ox, diag=O.diag(), X=np.stack(X))


# the knobs of the chain's schedule: a child gets exactly the ones of its setting
SCHEDULE_KNOBS = ["KVX_DEFER_U", "KVX_SYRK_DIRECT", "KVX_PAIR_TILES", "KVX_BLOCKED_GF", "KVX_U_STREAM", "KVX_SYRK_LDS_TILES", "KVX_FAR_WGS",
                  "KVX_U_BLOCK", "KVX_TWO_LEVEL_M", "KVX_OUTER_BLOCK", "KVX_SYRK128_TILES", "KVX_NO_GRAPH", "KVX_FACTOR_SUBTREES"]


def run_setting(setting, names, cache_dir, timeout=600):
    """one child process for one setting (dict of knobs); returns {matrix: {counts, err_l, res, digest}}"""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in SCHEDULE_KNOBS}
    env.update({k: str(v) for k, v in setting.items()})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), cache_dir] + list(names), env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (setting, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def total(res, key):
    return sum(v["counts"][key] for v in res.values())


# ---- the child ---------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def counts(reset=False):
    from kvxopt_amd._lib import lib, pi
    c = np.zeros(len(COUNTERS), dtype=np.int64)
    assert lib().kvx_dbg_syrk_counts(pi(c), 1 if reset else 0) == len(COUNTERS)
    return c


def check(name, cache_dir):
    import scipy.sparse as sp
    from kvxopt_amd import workloads
    from kvxopt_amd.chol import Factor
    n, cp, ri, v, perm, opts = matrix(name)
    ref = np.load(os.path.join(cache_dir, name + ".npz"))
    counts(reset=True)
    F = Factor(n, cp, ri, "L", perm, opts)
    assert np.array_equal(F.perm(), ref["perm"]), name
    B = _rhs(n)
    bits = []
    for rep in range(3):                                  # eager, capture, replay
        F.factorize(v)
        Lp, Li, Lx = F.get_factor()
        X = np.asfortranarray(B.copy())
        F.solve(X)
        bits.append((Lx.copy(), X))
    c = counts()
    for rep in (1, 2):
        assert np.array_equal(bits[rep][0], bits[0][0]), (name, "factor bits differ: eager vs call", rep)
        assert np.array_equal(bits[rep][1], bits[0][1]), (name, "solution bits differ: eager vs call", rep)
    # factor entries on the sparse pattern (the supernodal pattern holds explicit zeros the oracle does not store)
    A = sp.csc_matrix((Lx, Li, Lp), shape=(n, n))
    Om = sp.csc_matrix((ref["Ox"], ref["Oi"], ref["Op"]), shape=(n, n))
    scale = np.abs(ref["Ox"]).max()
    err_l = abs(A - Om).max() / scale
    assert err_l < 1e-11, (name, "factor", err_l)
    assert rel(F.diag(), ref["diag"]) < 1e-11, (name, "diag", rel(F.diag(), ref["diag"]))
    for s in range(9):
        X = np.asfortranarray(B.copy())
        F.solve(X, sys=s)
        if s in (6, 7, 8):
            assert np.array_equal(X, ref["X"][s]), (name, s)       # permutations / identity: bit exact
        else:
            assert rel(X, ref["X"][s]) < 5e-10, (name, s, rel(X, ref["X"][s]))
    X0 = bits[0][1]
    res = np.linalg.norm(workloads.sym_matvec(n, cp, ri, v, X0) - B) / np.linalg.norm(B)
    assert res < 1e-10, (name, "residual", res)
    digest = hashlib.sha256(bits[0][0].tobytes() + bits[0][1].tobytes()).hexdigest()
    return {"counts": dict(zip(COUNTERS, c.tolist())), "err_l": float(err_l), "res": float(res), "digest": digest}


def main():
    from kvxopt_amd import _lib
    _lib.require_device()
    cache_dir = sys.argv[1]
    out = {}
    for name in sys.argv[2:]:
        out[name] = check(name, cache_dir)
        print(name, json.dumps(out[name]["counts"]), "err %.2e res %.2e" % (out[name]["err_l"], out[name]["res"]), flush=True)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
