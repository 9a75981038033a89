"""Child process of test_chol_big_solve_gpu.py: one designed system of chol_big_solve_cases.py through the triangular sweeps of
the big fronts, under the KVX_FWD_NARROW_WGS of this process (the launcher reads it once per process, so every setting is a
process of its own; the parent sets it).  Prints one RESULT line.

The factor is built with OPTS and taken as the device holds it (get_factor); the references are numpy.longdouble substitutions
tree by tree.  Right-hand sides: the leading columns of one uniform(-1, 1) block, so that a column has one reference whatever
block it is solved in.  Routings:
  a  nrhs 1, 3     one grid layer per right-hand side (k_fwd_big_step, k_bwd_big_init, k_bwd_big_step); every column of the three
                   bit for bit its solo solve; the repeated call is a graph replay with the same bits
  b  nrhs 48, 65   the rhs-major kernels (k_wide_*_big_*): one ragged chunk; a full chunk and a chunk of one.  Three calls, same bits
  c  nrhs 64, 67   a second factor created under KVX_WIDE_FROM=0: the blocks of eight (67: a block of three) where the level is past
                   the workgroup threshold, the layered 64-row kernel elsewhere, the backward sweep in blocks of eight throughout;
                   columns 0, middle and last bit for bit their solo solves
  d  after a: a right-hand side scaled by 1e6, then the first one again: the bits of the first time (nothing stale in WK / W)
The crowds (11 000 to 17 000 rows) take 48 and 64 right-hand sides only in b and c: NRHS_CROWD.
Criteria: the launch counters equal expect_big on every first call (a replay counts nothing);
  sys 4 / 5   |B - L X| <= (nb + 1) 2^-53 |L| |X| componentwise, nb the order of the tree (check_substitution of test_chol_classes_gpu.py)
  sys 0       per column  max |x - ref| <= max(4 e64, 1e-13 max |ref|),  e64 the error of LAPACK dtrtrs on the same factor."""
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import chol_big_solve_cases as bc      # noqa: E402

KNOBS = ("KVX_FWD_NARROW_WGS", "KVX_WIDE_FROM", "KVX_NO_SUBTREES", "KVX_SUB_MAXF", "KVX_FACTOR_SUBTREES", "KVX_NO_GRAPH",
         "KVX_DBG_NO_SOLVE_GRAPH", "KVX_SOLVE_NOFORK", "KVX_GRAPH_SYNC_INSTANTIATE")
SETTINGS = {"default": {}, "rows256": {"KVX_FWD_NARROW_WGS": "0"}}
NRHS = {"a": (1, 3), "b": (48, 65), "c": (64, 67)}
NRHS_CROWD = {"a": (1, 3), "b": (48,), "c": (64,)}      # (the longdouble residuals of 11 000 to 17 000 rows x 64 columns take a second each)
TIMEOUT = 120


def nrhs_sets(name):
    return NRHS_CROWD if name in bc.CROWDS else NRHS


def run_child(setting, name):
    """one child for (setting, case); returns (returncode, result or None, output tail).  Raises subprocess.TimeoutExpired."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(SETTINGS[setting])
    env["KVX_GRAPH_SYNC_INSTANTIATE"] = "1"        # the call after the capture is then a replay for certain
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=env, capture_output=True, text=True, timeout=TIMEOUT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    return r.returncode, (json.loads(lines[-1][7:]) if lines else None), r.stdout[-3000:] + r.stderr[-3000:]


# ---- the child --------------------------------------------------------------------------------------------------------------------
def counters():
    from kvxopt_amd._lib import lib, pi
    out = np.zeros(len(bc.COUNTERS), dtype=np.int64)
    assert lib().kvx_dbg_chol_big_solve_counts(pi(out), 1) == len(bc.COUNTERS)
    return {c: int(v) for c, v in zip(bc.COUNTERS, out)}


def check(name):
    from kvxopt_amd import _lib
    from kvxopt_amd.chol import Factor
    _lib.require_device()
    t0 = time.time()
    case = bc.BY_NAME[name]
    e = os.environ.get("KVX_FWD_NARROW_WGS")
    narrow_wgs = int(e) if e is not None else bc.NARROW_WGS
    assert "KVX_WIDE_FROM" not in os.environ
    errors, ratios, hits, replays = [], {}, {c: 0 for c in bc.COUNTERS}, 0
    sets = nrhs_sets(name)
    ncol = max(max(v) for v in sets.values())
    n, cp, ri, vx = case.system()

    def factor():
        F = Factor(n, cp, ri, "L", opts=bc.OPTS)
        fr = bc.realised(F)
        assert sorted(fr[0]) == case.fronts, (name, "not the designed fronts")
        F.factorize(vx)
        Lp, Li, Lx = F.get_factor()
        return F, fr, (Lp, Li, Lx.copy())

    F, (fronts, level, parent, sup), (Lp, Li, Lx) = factor()
    perm = F.perm()
    ip = np.empty(n, dtype=np.int64)
    ip[perm] = np.arange(n)
    ranges = bc.tree_ranges(case, ip)
    stk = bc.stacks(bc.tree_blocks(Lp, Li, Lx, ranges), ranges)
    B = np.asfortranarray(np.random.default_rng(case.seed + 7).uniform(-1.0, 1.0, (n, ncol)))
    ref = {0: bc.solve_trees(stk, B, 0, perm, bc.subst_stack, bc.LD)}       # (sys 4 and 5 are held to their residuals)
    e64 = np.abs(bc.solve_trees(stk, B, 0, perm, bc.lapack_stack, np.float64).astype(bc.LD) - ref[0]).max(axis=0)
    floor = 1e-13 * np.abs(ref[0]).max(axis=0)
    t_ref = time.time() - t0

    def solve(H, Bin, s):
        X = np.asfortranarray(Bin.copy())
        H.solve(X, sys=s)
        return X

    def bound_ratio(X, s):
        r = X.shape[1]
        if s == 0:
            err = np.abs(X.astype(bc.LD) - ref[0][:, :r]).max(axis=0)
            return float((err / np.maximum(4.0 * e64[:r], floor[:r])).max())
        return bc.substitution_ratio(stk, B[:, :r], X, s == 5)

    def routed(H, routing, nrhs, s, form, calls):
        """the first call against the counters and the bound, the later ones against its bits; returns the first call's X"""
        nonlocal replays
        counters()
        X = solve(H, B[:, :nrhs], s)
        got = counters()
        want = bc.expect_big(fronts, level, s, nrhs, form, narrow_wgs)
        if got != want:
            errors.append((routing, "launches", "sys", s, "nrhs", nrhs, {k: (got[k], want[k]) for k in got if got[k] != want[k]}))
        for k, v in got.items():
            hits[k] += v
        rho = bound_ratio(X, s)
        key = "%s/sys%d" % (routing, s)
        ratios[key] = max(ratios.get(key, 0.0), rho)
        if not rho <= 1.0:
            errors.append((routing, "bound", "sys", s, "nrhs", nrhs, rho))
        for c in range(1, calls):
            Xc = solve(H, B[:, :nrhs], s)
            later = counters()
            if c >= 2 and not any(later.values()):
                replays += 1
            if c >= 2 and any(later.values()):
                errors.append((routing, "call %d enqueued launches: not a replay" % (c + 1), "sys", s, "nrhs", nrhs, later))
            if not np.array_equal(X, Xc):
                errors.append((routing, "call %d: other bits" % (c + 1), "sys", s, "nrhs", nrhs))
        return X

    def solo(H, routing, X, s, cols):
        for j in cols:
            if not np.array_equal(solve(H, B[:, j:j + 1], s)[:, 0], X[:, j]):
                errors.append((routing, "column %d of %d: not the bits of its solo solve" % (j, X.shape[1]), "sys", s))

    first = {}
    for s in (4, 5, 0):
        for nrhs in sets["a"]:
            X = routed(F, "a", nrhs, s, "rhs", 3)
            if nrhs == 1:
                first[s] = X
            else:
                solo(F, "a", X, s, range(nrhs))
        # d: a much larger right-hand side through the same workspaces, then the first one again
        big = solve(F, 1e6 * B[:, :1], s)
        if not np.abs(big).max() > 1e3 * np.abs(first[s]).max():
            errors.append(("d", "the scaled right-hand side was not solved", "sys", s))
        if not np.array_equal(solve(F, B[:, :1], s), first[s]):
            errors.append(("d", "stale workspace: other bits after a scaled solve", "sys", s))
        for nrhs in sets["b"]:
            routed(F, "b", nrhs, s, "wide", 3)
    t_ab = time.time() - t0

    os.environ["KVX_WIDE_FROM"] = "0"               # read at the device set-up of the next factor
    G, (fronts2, level2, _, _), (_, _, Lx2) = factor()
    assert fronts2 == fronts and level2 == level
    if not np.array_equal(Lx, Lx2):
        errors.append(("c", "the second factor has other bits"))
    for s in (4, 5, 0):
        for nrhs in sets["c"]:
            X = routed(G, "c", nrhs, s, "rhs", 2)
            solo(G, "c", X, s, (0, nrhs // 2, nrhs - 1))
            if not np.array_equal(X[:, 0], first[s][:, 0]):
                errors.append(("c", "column 0 of %d: not the bits of the first factor's solo solve" % nrhs, "sys", s))
    return {"case": name, "n": n, "narrow_wgs": narrow_wgs, "errors": errors, "ratios": ratios, "hits": hits, "replays": replays, "replays_wanted": 3 * (len(sets["a"]) + len(sets["b"])),
            "seconds": {"references": round(t_ref, 2), "a+b+d": round(t_ab, 2), "all": round(time.time() - t0, 2)}}


if __name__ == "__main__":
    try:
        out = check(sys.argv[1])
    except Exception:
        traceback.print_exc()
        sys.exit(1)
    print("RESULT " + json.dumps(out))
