"""Child process and shared helpers of the sparse-LU kernel-class tests (test_lu_classes_gpu.py, test_lu_bounds.py).

The routing knobs of the LU path (KVX_LU_WP, KVX_LU_WP_MAXCNT, KVX_LU_LDS_LEGACY, KVX_LU_UNBLOCKED, KVX_LU_GRAPH: lu_internal.hpp
LuKnobs, read when a numeric object is created; KVX_LU_NO_BTF: read by the analysis) hold for the life of a factor, so
every setting runs in a process of its own.  For each case named on the command line the child factors (klu.numeric), refactors
with values perturbed by +-5 % (the REUSE kernels), refactors twice more from the same buffers (capture, then replay of the launch
graph), and after every step checks the factor, the solves, the pivot rule and the structure against bounds that come from the
arithmetic alone (below) and to the CPU oracle, and reports the launch counters (kvx_dbg_lu_counts) of every step as one RESULT line.

Cases: "d<n><p>" is a dense block of order n given as a sparse matrix -- one diagonal block, one front of m = k = n -- with the
value pattern p: a = Gaussian, b = Gaussian with an exactly zero (stored) diagonal, c = strictly column diagonally dominant with a
unit diagonal that is also every row's largest entry (the row scaling is then exact and the dominance is that of the scaled
matrix, which elimination preserves: no interchange, max |L| <= 1, P = Q), e = as c with off-diagonal column sums 1e-4, analysed
as it is and factored with the rows of pivots 20 and n - 3 exchanged: exactly one interchange, in a known pivot block.  "mixed<p>", "many20<p>", "two_classes<p>" are block
diagonal matrices of such blocks; "bp_800" is the golden matrix.

Bounds (u = 2^-53, gamma_k = k u / (1 - k u); L, U, P, Q, R, F of klu.get_numeric, R P A Q = L U + F):
  factor  |R P A Q - (L U + F)| <= gamma_{n+2} |L| |U| entrywise (Higham, Accuracy and Stability, Thm 9.3, for any elimination order
          and any pivot choice; 2 more for the row scaling), dense for n <= 2100 (on 256 seeded columns above), sparse otherwise;
  solve   |R P b - (L U + F) Q'x| <= gamma_{3n+4} (|L| |U| + |F|) |Q'x| (Thm 9.4 with the scalings), mirrored for A'x = b;
  pivots  max |L_ij| <= (1 + 4u) / stol, stol = 1e-3 (lu_internal.hpp)."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U_ROUND = 2.0 ** -53
STOL = 1e-3
DENSE_MAX = 2100                      # above: the factor bound on 256 seeded columns (one front) or sparse (many fronts)
COUNTERS = (["wp%d" % t for t in range(8)] + ["tiled%d" % t for t in range(8)] +
            ["lds_legacy", "unblocked", "panel_reg32", "panel_reg16", "panel_reg8", "panel_lds", "panel_lds_work", "trsm",
             "trsm_skipped", "gemm", "fwd_small", "fwd_big", "bwd_small", "bwd_big"])
KNOBS = ["KVX_LU_WP", "KVX_LU_WP_MAXCNT", "KVX_LU_LDS_LEGACY", "KVX_LU_UNBLOCKED", "KVX_LU_GRAPH", "KVX_LU_NO_BTF"]
LDS_M, SOLVE_BIG_M = 112, 384

MULTI = {"mixed": [1500, 300, 120, 40],             # LDS and blocked fronts of different heights on one level
         "many20": [20] * 600,                       # more than 512 fronts of one class: the tiled kernel without any knob
         "two_classes": [10] * 300 + [40] * 300}     # more than 256 LDS fronts: one launch per class, alternating streams


def gamma(k):
    return k * U_ROUND / (1.0 - k * U_ROUND)


def lds_T(m):
    """template argument of the LDS kernels that serve a front of order m <= 112 (classes 16, 32, 48, 64, 88, 112)"""
    for c, t in ((16, 1), (32, 2), (48, 3), (64, 4), (88, 6), (112, 7)):
        if m <= c:
            return t
    raise ValueError(m)


def block_width(rows):
    """lu_symbolic.hpp lu_big_block_width"""
    return 32 if rows <= 1024 else (16 if rows <= 2048 else 8)


def panel_steps(max_m, max_k):
    """panel launches of one pass over a level whose tallest front has max_m rows and max_k pivots, by kernel"""
    out = {"panel_reg32": 0, "panel_reg16": 0, "panel_reg8": 0, "panel_lds": 0}
    jb = 0
    while jb < max_k:
        w = block_width(max_m - jb)
        out["panel_reg%d" % w] += 1
        out["panel_lds"] += max_m - jb > 4096
        jb += w
    return out


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
ONE_SWAP = (20, -3)                   # pattern e: the rows (second from the end of the block) that change places


def dense_block(n, pattern, seed, swapped=True):
    rng = np.random.default_rng([seed, n, ord(pattern)])
    D = rng.standard_normal((n, n))
    if pattern == "b":
        D[np.arange(n), np.arange(n)] = 0.0
    elif pattern == "c":
        D[np.arange(n), np.arange(n)] = 0.0
        s = np.abs(D).sum(axis=0)
        D *= 0.6 / np.where(s > 0, s, 1.0)                          # off-diagonal column sums 0.6, every entry below 0.6
        D[np.arange(n), np.arange(n)] = rng.choice([-1.0, 1.0], n)
    elif pattern == "e":
        D[np.arange(n), np.arange(n)] = 0.0
        D *= 1e-4 / np.abs(D).sum(axis=0)                           # off-diagonal column sums 1e-4: below stol times the diagonal
        D[np.arange(n), np.arange(n)] = rng.choice([-1.0, 1.0], n)
        if swapped:
            r1, r2 = ONE_SWAP[0], n + ONE_SWAP[1]
            D[[r1, r2]] = D[[r2, r1]]
    elif pattern != "a":
        raise KeyError(pattern)
    return D


def case_blocks(name):
    """name -> (orders of the dense diagonal blocks, pattern)"""
    if name[0] == "d" and name[1:-1].isdigit():
        return [int(name[1:-1])], name[-1]
    return MULTI[name[:-1]], name[-1]


def case_matrix(name, golden_dir=None, swapped=True):
    """name -> (n, colptr, rowind, values) with EVERY entry of the blocks stored, zeros included"""
    if name == "bp_800":
        z = np.load(os.path.join(golden_dir or os.path.join(ROOT, "tests", "golden"), "bp_800.npz"))
        return int(z["n"]), z["colptr"].astype(np.int64), z["rowind"].astype(np.int64), z["values"].astype(np.float64)
    orders, pattern = case_blocks(name)
    cnt, ri, v, off = [], [], [], 0
    for b, nb in enumerate(orders):
        D = dense_block(nb, pattern, 1000 + b if len(orders) > 1 else 7, swapped)
        cnt.append(np.full(nb, nb, dtype=np.int64))
        ri.append(np.tile(np.arange(off, off + nb, dtype=np.int64), nb))
        v.append(D.reshape(-1, order="F"))
        off += nb
    cp = np.concatenate([[0], np.cumsum(np.concatenate(cnt))]).astype(np.int64)
    return off, cp, np.concatenate(ri), np.concatenate(v)


def perturbed(v, seed=99):
    return v * (1.0 + 0.05 * np.random.default_rng(seed).uniform(-1.0, 1.0, v.size))


def rhs(n, nrhs):
    return np.asfortranarray(np.random.default_rng([n, nrhs]).standard_normal((n, nrhs)))


# ---- the bounds -------------------------------------------------------------------------------------------------------------------
class Factors:
    """L, U, F (scipy CSC), the pivotal row / column order p, q (R P A Q [i, j] = A[p[i], q[j]] / rs[i]) of one factorisation"""

    def __init__(self, n, L, U, F, p, q, rs):
        self.n, self.L, self.U, self.F, self.dense = n, L, U, F, None
        self.p, self.q, self.rs = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64), np.asarray(rs, dtype=np.float64)

    def key(self):
        h = hashlib.sha256()
        for a in (self.L.indptr, self.L.indices, self.L.data, self.U.indptr, self.U.indices, self.U.data, self.F.data, self.p, self.q, self.rs):
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()


def factors_from_get_numeric(n, out):
    import scipy.sparse as sp
    L, U, P, Q, R, F, r = out
    cs = lambda S: sp.csc_matrix((np.asarray(S.values, dtype=np.float64), S.rowind, S.colptr), shape=S.size)
    Pm, Qm, Rm = cs(P), cs(Q), cs(R)
    for M in (Pm, Qm):                                               # permutation matrices
        assert M.nnz == n and np.all(M.data == 1.0) and np.all(np.diff(M.indptr) == 1) and np.array_equal(np.sort(M.indices), np.arange(n))
    p = np.empty(n, dtype=np.int64); p[Pm.indices] = np.arange(n)    # P(i, p[i]) = 1, stored by columns
    q = Qm.indices.astype(np.int64)                                  # Q(q[i], i) = 1
    assert np.array_equal(Rm.indices, np.arange(n)) and np.all(np.diff(Rm.indptr) == 1)
    assert r[0] == 0 and r[-1] == n
    return Factors(n, cs(L), cs(U), cs(F), p, q, 1.0 / Rm.data), [int(x) for x in r]


def factors_from_oracle(n, O):
    import scipy.sparse as sp
    (Lp, Li, Lx), (Up, Ui, Ux), P, Q, Rs = O.extract()
    return Factors(n, sp.csc_matrix((Lx, Li, Lp), shape=(n, n)), sp.csc_matrix((Ux, Ui, Up), shape=(n, n)), sp.csc_matrix((n, n)), P, Q, Rs)


def worst_ratio(E, B):
    """max E / B over the entries, 0 where E is exactly 0; inf where the bound is missed by a nonzero error over a zero bound, or
    where either side is not a number (a NaN compares false with everything: it must not pass as a small error)"""
    E, B = np.asarray(E, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if E.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        R = E / B
    R[E == 0] = 0.0
    R[~np.isfinite(E) | ~np.isfinite(B) | np.isnan(R)] = np.inf
    return float(R.max())


def all_finite(fa):
    return all(np.all(np.isfinite(a)) for a in (fa.L.data, fa.U.data, fa.F.data, fa.rs))


def check_structure(fa):
    """L unit lower, U upper, p and q permutations; returns max |L_ij|"""
    import scipy.sparse as sp
    n = fa.n
    assert all_finite(fa), "L, U, F or the row scaling hold values that are not finite"
    assert abs(sp.triu(fa.L, 1)).sum() == 0 and np.all(fa.L.diagonal() == 1.0), "L is not unit lower triangular"
    assert abs(sp.tril(fa.U, -1)).sum() == 0, "U is not upper triangular"
    for w in (fa.p, fa.q):
        assert np.array_equal(np.sort(w), np.arange(n)), "not a permutation"
    return float(np.abs(fa.L.data).max())


def factor_ratio(A, fa):
    """max over the entries of |R P A Q - (L U + F)| / (gamma_{n+2} |L| |U|); A: scipy CSC.  An entry with an error and a zero
    bound gives inf."""
    n = fa.n
    g = gamma(n + 2)
    if not all_finite(fa):
        return float("inf")
    if n <= DENSE_MAX or fa.L.nnz > 20 * n:
        if n <= DENSE_MAX:
            cols = np.arange(n)
        else:
            cols = np.sort(np.random.default_rng(n).choice(n, 256, replace=False))
        wide = np.longdouble if n <= 256 else np.float64             # (the product itself rounds: exact enough in long double where cheap)
        Ld, Ud = fa.L.toarray().astype(wide), fa.U[:, cols].toarray().astype(wide)
        S = (A[fa.p][:, fa.q[cols]].toarray() / fa.rs[:, None]).astype(wide)
        E = np.abs(S - (Ld @ Ud + fa.F[:, cols].toarray()))
        B = g * (np.abs(Ld) @ np.abs(Ud))
        del Ld, Ud, S
        return worst_ratio(E, B)
    import scipy.sparse as sp
    S = sp.diags(1.0 / fa.rs) @ A[fa.p][:, fa.q]
    E = abs(S - (fa.L @ fa.U + fa.F)).tocsc()
    B = (g * (abs(fa.L) @ abs(fa.U))).tocsc()
    E.eliminate_zeros()
    if E.nnz == 0:
        return 0.0
    Bd = np.asarray(B[E.nonzero()]).ravel()
    Ed = np.asarray(E[E.nonzero()]).ravel()
    return worst_ratio(Ed, Bd)


def solve_ratio(fa, b, x, trans):
    """max over entries and right-hand sides of the solve residual / (gamma_{3n+4} (|L| |U| + |F|) |y|), y = Q'x or R^-1 P x"""
    n = fa.n
    g = gamma(3 * n + 4)
    if not (all_finite(fa) and np.all(np.isfinite(x))):
        return float("inf")
    wide = np.longdouble if n <= 256 else np.float64                 # (the residual itself rounds: long double where cheap)
    if fa.L.nnz > 20 * n and n <= 2 * DENSE_MAX:                     # dense blocks: dense products
        if fa.dense is None:
            fa.dense = (fa.L.toarray().astype(wide), fa.U.toarray().astype(wide), fa.F.toarray().astype(wide))
        L, Um, Fm = fa.dense
    else:
        wide = np.float64
        L, Um, Fm = fa.L, fa.U, fa.F
    x, b = x.astype(wide), b.astype(wide)
    if trans == "N":
        y, t = x[fa.q], b[fa.p] / fa.rs[:, None].astype(wide)
        res = np.abs(t - (L @ (Um @ y) + Fm @ y))
        bnd = abs(L) @ (abs(Um) @ np.abs(y)) + abs(Fm) @ np.abs(y)
    else:
        y, t = x[fa.p] * fa.rs[:, None].astype(wide), b[fa.q]
        res = np.abs(t - (Um.T @ (L.T @ y) + Fm.T @ y))
        bnd = abs(Um).T @ (abs(L).T @ np.abs(y)) + abs(Fm).T @ np.abs(y)
    return worst_ratio(res, g * np.asarray(bnd, dtype=np.float64))


def to_csc(n, cp, ri, v):
    import scipy.sparse as sp
    return sp.csc_matrix((v, ri, cp), shape=(n, n))


# ---- the parent's side ------------------------------------------------------------------------------------------------------------
def run_setting(setting, names, timeout=300):
    """one child process for one setting (dict of knobs); returns {case: result}"""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update({k: str(v) for k, v in setting.items()})
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(names), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (setting, r.returncode, r.stdout[-3000:] + r.stderr[-3000:])
    print(r.stdout)
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    errors = {k: v["error"] for k, v in res.items() if "error" in v}
    assert not errors, (setting, errors)
    return res


# ---- the child --------------------------------------------------------------------------------------------------------------------
def counts(reset=False):
    from kvxopt_amd._lib import lib, pi
    c = np.zeros(len(COUNTERS), dtype=np.int64)
    assert lib().kvx_dbg_lu_counts(pi(c), 1 if reset else 0) == len(COUNTERS)
    return dict(zip(COUNTERS, c.tolist()))


def check(name):
    from kvxopt_amd import klu
    from kvxopt_amd.base import spmatrix
    from oracle.kvx_oracle import OracleKLU
    t_start = time.time()
    n, cp, ri, v0 = case_matrix(name)
    single = name != "bp_800" and len(case_blocks(name)[0]) == 1
    pattern = None if name == "bp_800" else case_blocks(name)[1]
    graphs = os.environ.get("KVX_LU_GRAPH", "1")[0] != "0"
    # pattern e is analysed with its dominant entries on the diagonal (the matching is then the identity) and factored with two rows
    # exchanged: the front interchanges exactly once, at a known pivot
    v_sym = case_matrix(name, swapped=False)[3] if pattern == "e" else v0
    Fs = klu.symbolic(spmatrix.from_ccs(n, n, cp, ri, v_sym))
    if pattern == "e":
        # the rows that change places are those of the pivots ONE_SWAP in the analysis' own column order (read from a
        # factorisation of the matrix as analysed, which interchanges nothing)
        q0 = klu.numeric(spmatrix.from_ccs(n, n, cp, ri, v_sym), Fs).num.extract()["Q"]
        V = v_sym.reshape(n, n, order="F").copy()
        r1, r2 = int(q0[ONE_SWAP[0]]), int(q0[n + ONE_SWAP[1]])
        V[[r1, r2]] = V[[r2, r1]]
        v0 = V.reshape(-1, order="F")
    out = {"n": n, "steps": [], "factor_ratio": 0.0, "solve_ratio": 0.0, "max_l": 0.0}
    h = hashlib.sha256()
    Fn, last, O, prev_p = None, None, None, None
    for step, v in enumerate((v0, perturbed(v0), perturbed(v0))):
        A = spmatrix.from_ccs(n, n, cp, ri, v)
        As = to_csc(n, cp, ri, v)
        counts(reset=True)
        passes0 = Fn.num.info()["passes"] if Fn else 0
        replays0 = Fn.num.graph_replays() if Fn else 0
        pass_replays = 0
        if step == 0:
            Fn = klu.numeric(A, Fs)
        # a launch graph is captured when a key comes twice in a row and replayed from the call after; a refactorisation that
        # fell back to a full factorisation (other pivots: another key) sets that back by one call
        calls = 0 if step == 0 else (1 if step == 1 else 2 + (out["steps"][1]["passes"] > 1))
        for _ in range(calls):
            r0 = Fn.num.graph_replays()
            assert klu.numeric(A, Fs, Fn) is Fn
            pass_replays += Fn.num.graph_replays() - r0
        c_factor = counts(reset=True)
        info = Fn.num.info()
        if single:                                                    # the case tests the class it names
            assert info["nfront"] == 1 and info["max_front"] == n and info["max_pivot_block"] == n, (name, info)
        fa, r = factors_from_get_numeric(n, klu.get_numeric(A, Fs, Fn))
        max_l = check_structure(fa)
        assert max_l <= (1.0 + 4 * U_ROUND) / STOL, (name, step, "pivot rule", max_l)
        if pattern == "c":                                            # dominance survives elimination: no interchange at all
            assert max_l <= 1.0 and np.array_equal(fa.p, fa.q), (name, step, "interchange in a dominant matrix", max_l)
        if pattern == "e":                                            # one interchange, where the rows were exchanged
            assert max_l <= 1.0 and np.flatnonzero(fa.p != fa.q).tolist() == [ONE_SWAP[0], n + ONE_SWAP[1]], (name, step, np.flatnonzero(fa.p != fa.q))
        if pattern == "b":                                            # a zero cannot be the first pivot of its block
            for b0, b1 in zip(r, r[1:]):
                assert np.any(fa.p[b0:b1] != fa.q[b0:b1]), (name, step, "block without interchange", b0)
        key = fa.key()
        if last is None or key != last[0]:                            # (the same factors of the same matrix: the same figures)
            last = (key, factor_ratio(As, fa))
        fr = last[1]
        print("%s step %d factor ratio %.3e max|L| %.3e" % (name, step, fr, max_l), flush=True)
        assert fr <= 1.0, (name, step, "factor bound", fr)
        sr = 0.0
        if step < 2 or not np.array_equal(O_q, fa.q):                 # (step 2 has the values of step 1: the same oracle factors)
            O, O_q = OracleKLU(n, cp, ri, v, Q=fa.q), fa.q
        for nrhs in (1, 3):
            b = rhs(n, nrhs)
            for trans in "NT":
                x = np.asfortranarray(b.copy())
                klu.solve(A, Fs, Fn, x, trans=trans, nrhs=nrhs)
                h.update(x.tobytes())
                s = solve_ratio(fa, b, x, trans)
                print("%s step %d solve %s nrhs %d ratio %.3e" % (name, step, trans, nrhs, s), flush=True)
                assert s <= 1.0, (name, step, "solve bound", trans, nrhs, s)
                sr = max(sr, s)
                xo = O.solve(b, trans)
                d = float(np.abs(x - xo).max())
                print("%s step %d oracle %s nrhs %d diff %.3e of %.3e" % (name, step, trans, nrhs, d, 1e-9 * max(1.0, np.abs(xo).max())), flush=True)
                assert d <= 1e-9 * max(1.0, np.abs(xo).max()), (name, step, "oracle", trans, nrhs, d)     # (false for a NaN too)
        c_solve = counts(reset=True)
        out["steps"].append({"factor": c_factor, "solve": c_solve, "passes": info["passes"] - passes0, "pass_replays": pass_replays,
                             "replays": Fn.num.graph_replays() - replays0, "calls": max(calls, 1),
                             "same_pivots": bool(prev_p is not None and np.array_equal(prev_p, fa.p))})
        prev_p = fa.p
        out["factor_ratio"], out["solve_ratio"], out["max_l"] = max(out["factor_ratio"], fr), max(out["solve_ratio"], sr), max(out["max_l"], max_l)
    if graphs:
        assert out["steps"][2]["pass_replays"] >= 1, (name, "no graph replay in the steady state", out["steps"][2])
    else:
        assert Fn.num.graph_replays() == 0, (name, "graph replays with KVX_LU_GRAPH=0")
    out["info"] = Fn.num.info()
    out["digest"] = h.hexdigest()
    out["seconds"] = time.time() - t_start
    return out


def main():
    from kvxopt_amd import _lib
    _lib.require_device()
    out = {}
    for name in sys.argv[1:]:
        try:
            out[name] = check(name)
        except AssertionError as e:                                   # a missed check: reported, the other cases still run
            out[name] = {"error": repr(e)[:2000]}                     # (a device error is no AssertionError and ends the child)
            print(name, "FAILED", out[name]["error"], flush=True)
            continue
        print(name, "factor %.2e solve %.2e max|L| %.2e  %.1f s" % (out[name]["factor_ratio"], out[name]["solve_ratio"], out[name]["max_l"],
                                                                   out[name]["seconds"]), flush=True)
    print("RESULT " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
